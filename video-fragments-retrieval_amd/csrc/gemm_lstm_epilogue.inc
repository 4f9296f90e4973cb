// The gate epilogue of the fused LSTM step in gemm_nt_mfma_body (gemm.hip), as TEXT: included there once in place (TL = TI) and
// once inside the closure the inference step dispatches on its live block count -- see gemm_pipe_loop.inc for why.  Expects
// TL beside the names of the enclosing function; finishes the cells of the wave's first TL row blocks.
        // tile columns are (gate, unit): a lane holds i, f, g, o of unit 32*blockIdx.y + 16*wn + (lane & 15) in its four column
        // tiles, for 4*TI rows -- every cell is finished by ONE lane, no exchange
        const int H = g.lstm_H, unit = by * 32 + wn * 16 + l15;
        const bool valid = unit < H;
        // batched and branch-free: the previous cell state and the biases were requested at the head of the tile
        // (load_cell_inputs), here 4*TI independent gate evaluations
        // in ONE basic block (the asm pins the results ahead of the predicated stores; hipcc otherwise sinks each cell's ~190
        // instructions into its own store predicate, one serial dependency chain after the other)
        float cnew[TL][4], hnew[TL][4];
        float gsave[TRAIN ? TL : 1][4][4];
#pragma unroll
        for (int ti = 0; ti < TL; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ig = c_sigmoidf(acc[ti][0][r] + bi);
                const float fg = c_sigmoidf(acc[ti][1][r] + bf);
                const float gg = c_tanhf(acc[ti][2][r] + bg);
                const float og = c_sigmoidf(acc[ti][3][r] + bo);
                cnew[ti][r] = __builtin_fmaf(fg, cprev[ti][r], ig * gg);
                hnew[ti][r] = og * c_tanhf(cnew[ti][r]);
                asm volatile("" : "+v"(cnew[ti][r]), "+v"(hnew[ti][r]));
                if constexpr (TRAIN) { gsave[ti][r][0] = ig; gsave[ti][r][1] = fg; gsave[ti][r][2] = gg; gsave[ti][r][3] = og; }
            }
#pragma unroll
        for (int ti = 0; ti < TL; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + wm * (16 * TI) + ti * 16 + 4 * lq + r;
                if (valid && row < Mrows) {
                    if constexpr (MULTI) {
                        __hip_atomic_store(g.lstm_c + row * H + unit, cnew[ti][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(g.lstm_h + row * g.lstm_ldh + unit, hnew[ti][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else {
                    g.lstm_c[row * H + unit] = cnew[ti][r];
                    g.lstm_h[row * g.lstm_ldh + unit] = hnew[ti][r];
                    }
                    if constexpr (TRAIN) {
                        float *g4 = g.lstm_gates + row * 4 * H + unit;
                        g4[0] = gsave[ti][r][0]; g4[H] = gsave[ti][r][1]; g4[2 * H] = gsave[ti][r][2]; g4[3 * H] = gsave[ti][r][3];
                    }
                }
            }

// The software-pipelined K-tile loop of gemm_nt_mfma_body (gemm.hip), as TEXT: included there once in place (TL = TI, every
// row block of the wave) and once inside the closure the fused LSTM step dispatches on its live block count (TL = 0 .. TI).
// It is a file of its own because wrapping the in-place copy in a closure as well changes the register allocation and the
// instruction count of the dense and convolution kernels.  Expects TL / TLC (the blocks to compute, as a constant and as an
// integral_constant) beside the names of the enclosing function.
        float fa[RING][TL ? TL : 1], fb[RING][4];
        auto frag_read = [&](int buf, int slice, int slot) {
            if constexpr (TL > 0) {
            const float *As = lds + buf * BUF_FLOATS, *Ws = As + A_FLOATS;
            const float *ap = &As[lds_off(wm * (16 * TI) + l15, lq) + slice * 4];
            const float *wp = &Ws[lds_off(wn * 64 + l15, lq) + slice * 4];
#pragma unroll
            for (int ti = 0; ti < TL; ++ti) fa[slot][ti] = ap[ti * RBLK];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) fb[slot][tj] = wp[tj * RBLK];
            }
        };
        // the first K-tile's loads are in flight while the accumulators are initialised (C-in / the LSTM table gather: two
        // dependent load rounds whose latency would otherwise stand alone at the head of every tile)
        if (nk > 0) gload_main(0);
        init_acc(TLC);
        // (fused LSTM step: the gate epilogue's loads ride in the same latency window; nothing in the other kernels)
        load_cell_inputs(TLC);
        // Accumulators that start from LOADED values (C-in, the LSTM projection-table gather) must have landed before the loop is
        // entered: otherwise the waitcnt pass, merging the loop-entry state into the loop header, guards the first MFMAs of EVERY
        // trip with vmcnt(3) .. vmcnt(0) -- which on the back edge drains the staging loads requested five slices earlier, i.e. the
        // prefetch is thrown away every second K-tile (seen in the ISA of lstm_step_mfma_pair).  The values are needed by the
        // first MFMA anyway; waiting here, before K-tile 1 is requested, costs nothing.
        // (unconditional: behind a run-time test the wait would itself sit on one arm of a join)
        __builtin_amdgcn_s_waitcnt(0x0F70);                                                    // vmcnt(0)
        if (nk > 0) {
            swrite(0);
            gload_main((nk > 1 ? 1 : 0) * MBK);
        }
        __syncthreads();
        GSTAMP(0)
        if (nk > 0) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) frag_read(0, d, d % RING);
        }
        // two K-tiles per trip, so the LDS buffer of every read and write is a compile-time constant and folds into the
        // instruction's immediate offset (a run-time buffer index cost 10-15 vector adds per K-tile)
        auto ktile = [&](int kt, auto cbc) {
            constexpr int cb = decltype(cbc)::value, nb = cb ^ 1;
#pragma unroll
            for (int k4 = 0; k4 < NS; ++k4) {
                const int sn = k4 + DEPTH;                   // slice whose fragments are fetched now
#ifndef VFR_GEMM_NOSYNC
                if (sn == NS) __syncthreads();               // K-tile kt+1 (written at slice 1) is visible from here on
#endif
                if (sn < NS) frag_read(cb, sn, sn % RING);
                else         frag_read(nb, sn - NS, sn % RING);    // (past the last K-tile: stale data, never used)
                __builtin_amdgcn_sched_barrier(0);
                // SPREAD: the staging stores of K-tile kt + 1 go out ONE behind each MFMA of slices 1 and 2 instead of as a
                // block behind slice 1 (a wave alone on its SIMD issues no MFMA while it moves 5-8 float4 to the LDS: 254 cycles
                // per K-tile of a 32-row tile)
                constexpr int NM = TL * 4, NPIECE = NA + NW;
                static_assert(TL < TI || NPIECE <= 2 * NM, "staging pieces must fit behind the MFMAs of two slices");
                constexpr bool SPREAD = NPIECE <= 2 * NM;      // (too few live MFMAs to hang the pieces on: one block)
#pragma unroll
                for (int ti = 0; ti < TL; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 4; ++tj) {
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[k4 % RING][ti], fb[k4 % RING][tj], acc[ti][tj], 0, 0, 0);
                        if (SPREAD && (k4 == 1 || k4 == 2)) {
                            const int piece = (k4 - 1) * NM + ti * 4 + tj;
                            if (piece < NPIECE) swrite_piece(nb, piece);
                        }
                    }
                // (pin the order: MFMA, [the piece's zero-selects], its LDS store -- left alone the scheduler hangs four of the stores
                // behind the first MFMA)
                if (SPREAD && (k4 == 1 || k4 == 2)) {
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const int piece = (k4 - 1) * NM + m;
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (piece < NPIECE) {
                            if (((CONV && !CHALO) || (LSTM && !LFAST)) && piece < NA) __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (!SPREAD && k4 == 1) swrite(nb);
                if (k4 == GLOAD_SLICE) gload_main((kt + 2 < nk ? kt + 2 : nk - 1) * MBK);
            }
        };
        int kt = 0;
        for (; kt + 1 < nk; kt += 2) {
            ktile(kt, std::integral_constant<int, 0>{});
            ktile(kt + 1, std::integral_constant<int, 1>{});
        }
        if (kt < nk) ktile(kt, std::integral_constant<int, 0>{});

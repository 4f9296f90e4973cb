// Host-side seams between the scorer's translation units.  Without relocatable device code a kernel can only be launched
// from the unit that defines it, so the units share HOST functions (and the workspace layouts those functions work on),
// never kernel declarations.  Every function here is defined in exactly one unit, named at its declaration.
#pragma once
#include "vfr_common.h"

namespace vfr {

inline int kpl_for(int k) { return k <= 128 ? 4 : 8; }   // keys per lane of the wave sorts: pools of 256 or 512 keys

// ---- MFMA pre-filter workspace (score.hip; layout and guard described in score_mfma.h) ----
struct BankSig;
struct MfmaWs {
    float *rv; BankSig *sig; unsigned long long *hash_now; int *stale; int *fallback; unsigned long long *pairs_total; unsigned long long *cnt_ws; size_t zero_bytes; char *zero_base;
    float *va; float4 *qmeta; unsigned *tab; unsigned *wmax, *qbound; unsigned short *vb; ulonglong2 *amb; int tasks, groups;
    float *mu, *vc, *qc; double *mean_partial; int mean_blocks, mean_rows;
    signed char *vl, *ql; float2 *mean_minmax; double *bankc; float *qf; double2 *qdbg; double *qscale;   // int8 operand mode
    void *topk; size_t topk_bytes; size_t total;
    int *perm, *diff; unsigned *hist; uint2 *hrange; float *Qs, *rds; int64_t *ris, *seeds, *cnts; float *ods; int64_t *ois;
};
MfmaWs carve_mfma(void *base, int64_t Nq, int Nv, int total_clips, int k);
// the front of that workspace, whose offsets depend on total_clips alone, as the video-level units carve it: a workspace shared
// with vfr_score_topk_mfma keeps the bank-side products valid for both (VFR_MFMA_BANK_READY).  Those units have no int8 mode:
// their MfmaWs carries no min/max and no constants buffer
MfmaWs carve_bank_front(void *base, int total_clips);

// The bank-side pre-pass (score.hip): hash, signature check (guard of BANK_READY), mean partial and final, then the centred rows
// as fp32 (with the bf16 copy when `bf16`) or as int8 limbs (`i8`).  Launches only: zero-fills, the query side, the profiler
// scope and the launch check stay with the caller.
void bank_prepass(MfmaWs &mw, const float *V, const int32_t *clip_offsets, int Nv, int total_clips, int D, float eps, bool bank_ready,
                  bool bf16, bool i8, hipStream_t st);
// the fast path's pre-pass of the video-level units (score.hip, next to mfma_prep_q_kernel): the zero-fill of the guard's words,
// bank_prepass without bf16 / int8, then the centred query rows and their meta
int vtk_prepass(MfmaWs &mw, float *qc, float4 *qmeta, const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets,
                int Nv, int total_clips, int D, float eps, bool bank_ready, hipStream_t st);

// ---- a handful of queries (score_smallq.hip) ----
bool smallq_applicable(int64_t Nq, int Nv, int total_clips, int max_clips, int num_rank, int k);
size_t smallq_workspace_bytes(int64_t Nq, int total_clips, int k);   // 0 above the path's query limit
int run_smallq(const float *Q, int64_t Nq, const float *V, const int32_t *clip_offsets, const int64_t *moment_offsets, int Nv,
               int total_clips, int max_clips, int D, float eps, int64_t id_base, int k, float *out_dist, int64_t *out_idx, int num_rank,
               const float *rank_dist, const int64_t *rank_idx, int64_t *count_lt, void *workspace, vfr_stream_t stream);

}  // namespace vfr

// tg_spot_topk.h -- each spot's k most probable cells straight from the logits: the COLUMN reading of the mapping (which cells sit in
// a spot: deconvolution, per-spot cell lists), V x k (value, cell) pairs instead of the dense C x V plane of tg_softmax_out and a
// strided host sort over its columns.  The row-wise lists of tg_topk.h cannot answer it: a spot's strongest cell need not have that
// spot among its own k best.
//
//   tg_spot_topk<KL, SUM>   a 256-thread workgroup takes a strip of TG_SPOT_STRIP = 256 adjacent spots x a slab of `slab_rows` cells
//                           (grid: strips x slabs).  A thread owns ONE column: it walks the slab's rows in ascending order,
//                           TG_SPOT_UNROLL = 8 rows' loads issued before the first use (a wave reads 256 contiguous bytes of a row per
//                           load; each logit is read from HBM once, non-temporally), forms p = tg_exp(M[c][v] - rshift[c]) * rinvz[c]
//                           -- the expression of tg_softmax_out, so the values are the bits tg_mapper_result writes; rshift[c] and
//                           rinvz[c] are the same for the whole workgroup (scalar loads) -- and keeps the best KL entries of its
//                           column in registers: key[KL] / cell[KL], sorted, indexed by fully unrolled loops only (KL is a template
//                           argument: 1, 4, 8, 16, 32 -- the smallest one >= k runs), so nothing lands in scratch.
//                           Order: value descending, equal values to the LOWER cell, decided on p, never on M: the entry is the word
//                           {bits(p) + 1, ~c} of tg_topk.h, kept here as its two halves.  The rows arrive in ascending order, so a
//                           new element of equal key always loses: ONE 32-bit compare `key > key[KL - 1]` rejects an element that
//                           does not enter; one that does is placed by an unrolled shift (2 compares and 4 selects per position).
//                           Key 0 is "no entry": a column with fewer admitted cells than k ends in (0.0f, -1).  Threads of the
//                           columns V .. 256 * strips - 1 leave at once: padding columns are never read and never written.
//                           Constrained mode: a cell takes part only if its gate f_c > min_filter (`gate` non-null; the branch is
//                           uniform).  SUM: the column sum of p over the admitted cells, every term converted to fp64 and added in
//                           ascending row order -> colpart[slab][v]; without SUM the kernel holds no fp64 instruction.
//                           The slab's list goes to val / cell [V][ld] at column slab * k .. slab * k + k - 1 (one slab: ld = k, these
//                           ARE the outputs).
//   tg_topk_merge_rows      (tg_topk.h, unchanged) one launch over n_rows = V, n_in = slabs * k merges the slabs' lists: value
//                           descending, then cell ascending, pad index -1 behind everything -- the order above.
//   tg_spot_colsum_finish   colsum[v] = (float)(colpart[0][v] + colpart[1][v] + ...): the slabs in ascending order in fp64, rounded once.
// No global atomics, no polling, no LDS; nothing of the handle's state or workspace is written.
#pragma once
#include "tg_device.h"
#include "tg_topk.h"

#define TG_SPOT_TOPK_MAX 32                             // largest k: tg_spot_topk<32, true> takes 83 VGPRs, 6 waves per SIMD, no scratch
#define TG_SPOT_STRIP 256                               // spots per workgroup, one per thread
#define TG_SPOT_UNROLL 8                                // rows whose loads are in flight together; the smallest slab height accepted
#define TG_SPOT_MIN_SLAB 256                            // the library never chooses a slab shorter than this ...
#define TG_SPOT_TARGET_WGS 1024                         // ... and aims at this many workgroups: 4 per CU, one wave of each on every SIMD
#define TG_SPOT_MAX_SLABS 65535                         // (blockIdx.y)

struct TgSpotTopkArgs {
    const float *M, *rshift, *rinvz;
    const float* gate;                                  // [C] the filter values f_c, or null: every cell takes part
    float min_filter;
    int C, V, Vp, k, slab_rows;
    long long ld;                                       // entries per spot of val / cell: slabs * k
    float* val;                                         // [V][ld]
    int* cell;                                          // [V][ld]
    double* colpart;                                    // [slabs][V] (SUM only)
};

// slab height: the caller's, or (0) the smallest multiple of TG_SPOT_UNROLL >= TG_SPOT_MIN_SLAB that keeps strips x slabs at or below
// TG_SPOT_TARGET_WGS workgroups -- 30 000 x 10 000: 40 strips, 25 slabs of 1 200 rows, 1 000 workgroups
TG_HD int tg_spot_topk_slab_rows(int C, int V, int slab_rows) {
    if (slab_rows > 0) return slab_rows;
    const int strips = (V + TG_SPOT_STRIP - 1) / TG_SPOT_STRIP;
    const int want = TG_SPOT_TARGET_WGS / strips > 0 ? TG_SPOT_TARGET_WGS / strips : 1;
    int rows = (C + want - 1) / want;
    if (rows < TG_SPOT_MIN_SLAB) rows = TG_SPOT_MIN_SLAB;
    return (rows + TG_SPOT_UNROLL - 1) / TG_SPOT_UNROLL * TG_SPOT_UNROLL;
}
TG_HD int tg_spot_topk_list_len(int k) { return k <= 1 ? 1 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

static inline TgShape tg_spot_topk_shape(int V, int n_slabs) { return tg_shape((V + TG_SPOT_STRIP - 1) / TG_SPOT_STRIP, n_slabs, TG_SPOT_STRIP, 0); }
static inline TgShape tg_spot_merge_shape(int V) { return tg_shape(V, 1, 256, TG_TOPK_LDS); }          // tg_topk_merge_rows over the spots
static inline TgShape tg_spot_colsum_finish_shape(int V) { return tg_shape((V + 255) / 256, 1, 256, 0); }

template <int KL, bool SUM> TG_KERNEL void TG_LAUNCH_BOUNDS(TG_SPOT_STRIP) tg_spot_topk(TgSpotTopkArgs a) {
    const int v = blockIdx.x * TG_SPOT_STRIP + threadIdx.x;
    if (v >= a.V) return;                                               // (no barrier below)
    const int slab = blockIdx.y;
    const int c0 = slab * a.slab_rows;
    const int c1 = a.C - c0 < a.slab_rows ? a.C : c0 + a.slab_rows;
    const float* col = a.M + v;
    const size_t pitch = (size_t)a.Vp;
    unsigned key[KL];
    int cell[KL];
#pragma unroll
    for (int i = 0; i < KL; ++i) { key[i] = 0u; cell[i] = -1; }
    double sum = 0.0;
    // one element of row c: x is its logit
    auto admitted = [&](int c) { return !a.gate || a.gate[c] > a.min_filter; };       // (uniform)
    auto take = [&](float x, int c, float sh, float iz) {
        const float p = tg_exp(x - sh) * iz;
        if (SUM) sum += (double)p;
        const unsigned kk = __builtin_bit_cast(unsigned, p) + 1u;
        if (kk > key[KL - 1]) {                                         // an equal key has the larger cell index: it stays out
#pragma unroll
            for (int i = KL - 1; i >= 1; --i) {
                const bool up = kk > key[i - 1], here = kk > key[i];    // above entry i - 1: that one moves down; else between the two
                cell[i] = up ? cell[i - 1] : (here ? c : cell[i]);
                key[i] = up ? key[i - 1] : (here ? kk : key[i]);
            }
            if (kk > key[0]) { key[0] = kk; cell[0] = c; }
        }
    };
    int c = c0;
    for (; c + TG_SPOT_UNROLL <= c1; c += TG_SPOT_UNROLL) {
        float x[TG_SPOT_UNROLL], sh[TG_SPOT_UNROLL], iz[TG_SPOT_UNROLL];
        bool in[TG_SPOT_UNROLL];
#pragma unroll
        for (int u = 0; u < TG_SPOT_UNROLL; ++u) x[u] = tg_ld_stream<true>(col + (size_t)(c + u) * pitch);
#pragma unroll
        for (int u = 0; u < TG_SPOT_UNROLL; ++u) { sh[u] = a.rshift[c + u]; iz[u] = a.rinvz[c + u]; in[u] = admitted(c + u); }   // the rows' constants: one wait
#pragma unroll
        for (int u = 0; u < TG_SPOT_UNROLL; ++u)
            if (in[u]) take(x[u], c + u, sh[u], iz[u]);
    }
    for (; c < c1; ++c)
        if (admitted(c)) take(tg_ld_stream<true>(col + (size_t)c * pitch), c, a.rshift[c], a.rinvz[c]);
    const size_t at = (size_t)v * (size_t)a.ld + (size_t)slab * (size_t)a.k;
#pragma unroll
    for (int r = 0; r < KL; ++r)
        if (r < a.k) {
            const bool real = key[r] != 0u;
            a.val[at + r] = real ? __builtin_bit_cast(float, key[r] - 1u) : 0.f;
            a.cell[at + r] = real ? cell[r] : -1;
        }
    if (SUM) a.colpart[(size_t)slab * a.V + v] = sum;
}

TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_spot_colsum_finish(const double* colpart, int n_slabs, int V, float* colsum) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    double s = 0.0;
    for (int j = 0; j < n_slabs; ++j) s += colpart[(size_t)j * V + v];
    colsum[v] = (float)s;
}

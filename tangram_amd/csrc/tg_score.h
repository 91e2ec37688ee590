// tg_score.h -- every gene's cosine score between a predicted and a measured spots x genes plane: what compare_spatial_geneexp reports
// (reference tangram/utils.py:424-426, one np.linalg.norm pair and one dot per gene on the host) without a plane copied to the host.
// n_spots x n_genes go in twice, n_genes numbers come out: a pure streaming reduction whose floor is the bytes of the two planes.
//
//   tg_score_partials<VEC>  a 256-thread workgroup per (strip of TG_SCORE_STRIP gene columns) x (slab of TG_SCORE_SLAB spot rows).  Genes
//                        are the contiguous axis: a wave reads WHOLE rows of the strip -- 64 lanes x 16 bytes = 1 KB per plane and row --
//                        and wave w takes the TG_SCORE_RPW rows slab + w TG_SCORE_RPW ... of the slab in ascending order,
//                        TG_SCORE_BATCH rows of both planes loaded (non-temporal: every element is read once) before the first use.
//                        A lane owns four gene columns and their twelve sums: x = (double)pred, y = (double)meas,
//                        dot += x y, pp += x x, gg += y y as fp64 fma -- the product of two fp32 values is exact in fp64, so each
//                        step is ONE rounding, that of the sum.  The four waves combine through LDS in wave order,
//                        ((w0 + w1) + w2) + w3, -> part[slab][3][n_genes].
//                          VEC     both planes 16-byte aligned, both pitches multiples of 4: lane l holds the genes 4 l .. 4 l + 3 of the
//                                  strip, one 16-byte load per plane and row (a quad that crosses n_genes is read element by element:
//                                  nothing behind n_genes is touched);
//                          scalar  any pitch and alignment: lane l holds the genes l, 64 + l, 128 + l, 192 + l, four coalesced
//                                  4-byte loads per plane and row.
//                        Which lane holds a gene does not enter its sums: a gene's chain is its rows in the order above, whatever
//                        the path, the strip, the column position, the pitches or n_genes -- the same column gives the same bits
//                        in any block of any call.  The order depends on n_spots alone (through the slabs).
//   tg_score_finish      TG_SCORE_FIN_GENES genes per 256-thread workgroup: TG_SCORE_FIN_TPG threads per gene fetch one slab each per
//                        round (the loads run side by side), then ONE thread per gene and moment adds the round's slabs to its sum in
//                        ASCENDING slab order -> moments[3][n_genes] (dot, pp, gg) and score = dot / (sqrt(pp) sqrt(gg)) in fp64
//                        (IEEE square root and division).  A zero norm gives 0 / 0 = NaN, as the reference does.
//   tg_score_merge       spot shards: the moments[3][n_genes] of W ranks, gathered -> their sums in ascending rank order and the score of
//                        the whole plane, formed as tg_score_finish forms it (at the end of this file).
// No atomics, fixed orders: the same inputs give the same bits on every call.  Rows and columns outside the planes enter as
// fma(0, 0, sum) = sum, which changes no bit (a sum starts at +0 and never becomes -0).
#pragma once
#include "tg_device.h"

#define TG_SCORE_STRIP 256                              // gene columns of a workgroup: a wave row of 64 lanes x TG_SCORE_VEC floats
#define TG_SCORE_VEC 4                                  // floats of a 16-byte load
#define TG_SCORE_SLAB 64                                // spot rows of a workgroup
#define TG_SCORE_RPW 16                                 // rows of a wave
#define TG_SCORE_BATCH 8                                // rows in flight per wave and plane
#define TG_SCORE_FIN_GENES 16                           // tg_score_finish: genes per workgroup
#define TG_SCORE_FIN_TPG 16                             //                  threads per gene = slabs per round
static_assert(TG_SCORE_STRIP == 64 * TG_SCORE_VEC && TG_SCORE_SLAB == 4 * TG_SCORE_RPW && TG_SCORE_RPW % TG_SCORE_BATCH == 0, "4 waves, whole batches");
static_assert(TG_SCORE_FIN_GENES * TG_SCORE_FIN_TPG == 256 && 3 * TG_SCORE_FIN_GENES <= 256, "one workgroup of tg_score_finish");
#define TG_SCORE_PART_LDS (4 * 3 * TG_SCORE_STRIP * 8)                                              // [4 waves][3][strip] doubles
#define TG_SCORE_FIN_LDS ((2 * 3 * TG_SCORE_FIN_TPG * TG_SCORE_FIN_GENES + 3 * TG_SCORE_FIN_GENES) * 8)    // [2][3][tpg][genes] + [3][genes]

TG_HD long long tg_score_strips(long long n_genes) { return (n_genes + TG_SCORE_STRIP - 1) / TG_SCORE_STRIP; }
TG_HD long long tg_score_slabs(long long n_spots) { return (n_spots + TG_SCORE_SLAB - 1) / TG_SCORE_SLAB; }
// the workspace: part[n_slabs][3][n_genes] doubles
TG_HD size_t tg_score_bytes(long long n_spots, long long n_genes) { return ((size_t)tg_score_slabs(n_spots) * 3 * (size_t)n_genes * 8 + 255) / 256 * 256; }

struct TgScoreArgs {
    const float* pred;
    const float* meas;
    long long ld_pred, ld_meas;
    int n_spots, n_genes, n_strips;
    double* part;                                       // [n_slabs][3][n_genes]
};

// place in the strip of element e of lane `lane`
template <bool VEC> TG_DEV int tg_score_col(int lane, int e) { return VEC ? TG_SCORE_VEC * lane + e : 64 * e + lane; }

// the lane's four elements of one row; g0: first gene of the strip
template <bool VEC> TG_DEV f32x4 tg_score_load(const float* row, int g0, int lane, int n_genes) {
    if (VEC && g0 + TG_SCORE_VEC * lane + TG_SCORE_VEC - 1 < n_genes) return tg_ld_stream<true>((const f32x4*)(row + g0 + TG_SCORE_VEC * lane));
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < TG_SCORE_VEC; ++e) {
        const int g = g0 + tg_score_col<VEC>(lane, e);
        if (g < n_genes) x[e] = tg_ld_stream<true>(row + g);
    }
    return x;
}

static inline TgShape tg_score_partials_shape(long long n_strips, long long n_slabs) { return tg_shape(n_strips * n_slabs, 1, 256, TG_SCORE_PART_LDS); }

template <bool VEC> TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_score_partials(TgScoreArgs a) {
    TG_LDS_DECL;
    double* wsum = (double*)tg_lds;                                     // [4][3][TG_SCORE_STRIP]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int strip = (int)(blockIdx.x % (unsigned)a.n_strips), slab = (int)(blockIdx.x / (unsigned)a.n_strips);   // (neighbouring workgroups: neighbouring strips of the same rows)
    const int g0 = strip * TG_SCORE_STRIP;
    const int row0 = slab * TG_SCORE_SLAB + wave * TG_SCORE_RPW;
    int nrows = a.n_spots - row0;                                       // rows of this wave: 0 .. TG_SCORE_RPW (wave-uniform)
    nrows = nrows < 0 ? 0 : (nrows > TG_SCORE_RPW ? TG_SCORE_RPW : nrows);
    const float* prow = a.pred + (size_t)row0 * (size_t)a.ld_pred;
    const float* mrow = a.meas + (size_t)row0 * (size_t)a.ld_meas;
    double acc[3][TG_SCORE_VEC];
#pragma unroll
    for (int e = 0; e < TG_SCORE_VEC; ++e) acc[0][e] = acc[1][e] = acc[2][e] = 0.0;
    for (int r0 = 0; r0 < nrows; r0 += TG_SCORE_BATCH) {
        f32x4 p[TG_SCORE_BATCH], m[TG_SCORE_BATCH];
#pragma unroll
        for (int i = 0; i < TG_SCORE_BATCH; ++i) {
            p[i] = m[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r0 + i < nrows) {
                p[i] = tg_score_load<VEC>(prow + (size_t)(r0 + i) * (size_t)a.ld_pred, g0, lane, a.n_genes);
                m[i] = tg_score_load<VEC>(mrow + (size_t)(r0 + i) * (size_t)a.ld_meas, g0, lane, a.n_genes);
            }
        }
#pragma unroll
        for (int i = 0; i < TG_SCORE_BATCH; ++i)                        // ascending rows: the order of every gene's three chains
#pragma unroll
            for (int e = 0; e < TG_SCORE_VEC; ++e) {
                const double x = (double)p[i][e], y = (double)m[i][e];
                acc[0][e] = __builtin_fma(x, y, acc[0][e]);
                acc[1][e] = __builtin_fma(x, x, acc[1][e]);
                acc[2][e] = __builtin_fma(y, y, acc[2][e]);
            }
    }
    // ---- the four waves in order
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int e = 0; e < TG_SCORE_VEC; ++e) wsum[(wave * 3 + j) * TG_SCORE_STRIP + tg_score_col<VEC>(lane, e)] = acc[j][e];
    __syncthreads();
    const int g = g0 + t;
    if (g < a.n_genes) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double* w = wsum + j * TG_SCORE_STRIP + t;
            a.part[((size_t)slab * 3 + j) * (size_t)a.n_genes + g] =
                ((w[0] + w[3 * TG_SCORE_STRIP]) + w[6 * TG_SCORE_STRIP]) + w[9 * TG_SCORE_STRIP];
        }
    }
}

static inline TgShape tg_score_finish_shape(long long n_genes) {
    return tg_shape((n_genes + TG_SCORE_FIN_GENES - 1) / TG_SCORE_FIN_GENES, 1, 256, TG_SCORE_FIN_LDS);
}

// part [n_slabs][3][n_genes] -> moments [3][n_genes] (or null), score [n_genes] (or null)
TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_score_finish(const double* part, int n_slabs, int n_genes, double* moments, double* score) {
    TG_LDS_DECL;
    constexpr int NG = TG_SCORE_FIN_GENES, TPG = TG_SCORE_FIN_TPG;
    double* buf = (double*)tg_lds;                                      // [2][3][TPG][NG]: a round's slabs, two copies by round parity: ONE barrier per round
    double* fin = buf + 2 * 3 * TPG * NG;                               // [3][NG]
    const int t = threadIdx.x, l = t % NG, q = t / NG;                  // fetching: slab q of the round; adding (t < 3 NG): moment q
    const int g = blockIdx.x * NG + l;
    const bool adds = t < 3 * NG;
    double acc = 0.0;
    int phase = 0;
    for (int s0 = 0; s0 < n_slabs; s0 += TPG, phase ^= 1) {
        double* b = buf + phase * 3 * TPG * NG;
        const int s = s0 + q;
        const bool live = s < n_slabs && g < n_genes;
#pragma unroll
        for (int j = 0; j < 3; ++j) b[(j * TPG + q) * NG + l] = live ? part[((size_t)s * 3 + j) * (size_t)n_genes + g] : 0.0;
        __syncthreads();
        if (adds) {
            const int n = n_slabs - s0 < TPG ? n_slabs - s0 : TPG;
            for (int u = 0; u < n; ++u) acc += b[(q * TPG + u) * NG + l];       // ascending slabs
        }
    }
    if (adds) {
        fin[q * NG + l] = acc;
        if (moments && g < n_genes) moments[(size_t)q * (size_t)n_genes + g] = acc;
    }
    __syncthreads();
    if (score && t < NG && g < n_genes) score[g] = fin[l] / (sqrt(fin[NG + l]) * sqrt(fin[2 * NG + l]));
}

// ---- spot shards: every rank reduces its own rows to moments[3][n_genes] (tg_score_finish), the W sets are gathered, and this kernel
// merges them: a thread per gene adds each of its three moments over the ranks in ASCENDING rank order, starting from rank 0's value
// (not from 0: one rank returns its bits), and ends as tg_score_finish ends.  Neighbouring threads read neighbouring doubles.
// in [W][3][n_genes] -> moments [3][n_genes] (or null), score [n_genes] (or null)
static inline TgShape tg_score_merge_shape(long long n_genes) { return tg_shape((n_genes + 255) / 256, 1, 256, 0); }

TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_score_merge(const double* in, int n_ranks, int n_genes, double* moments, double* score) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_genes) return;
    const size_t n = (size_t)n_genes;
    double s[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = in[(size_t)j * n + (size_t)g];
    for (int r = 1; r < n_ranks; ++r) {                                 // ascending ranks
        const double* p = in + (size_t)r * 3 * n + (size_t)g;
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] += p[(size_t)j * n];
    }
    if (moments) {
#pragma unroll
        for (int j = 0; j < 3; ++j) moments[(size_t)j * n + (size_t)g] = s[j];
    }
    if (score) score[g] = s[0] / (sqrt(s[1]) * sqrt(s[2]));
}

// tg_consist.h -- how well R repeated mappings of one problem agree, straight from the logits: what the tuning driver reports per
// trial (reference tangram/mapping_parameter_tuning.py:42-82, :133-139) without a cells x spots plane written, copied to the host or
// stacked into an fp64 cube there (30 000 x 10 000, three seeds: 3 x 1.2 GB of copies and a 7.2 GB one-hot cube for three
// correlations and two numbers per cell).
//
//   tg_consist_rows<R, MODE>  a 256-thread workgroup per row of R planes of one shape (n_rows x n_cols, row pitch ld); beyond
//                        TG_CONSIST_MAX_PARTS rows workgroup b takes the rows b, b + grid, ...  MODE says where an element p comes from; everything behind the load is ONE body, so equal values give equal bits:
//                          TG_CONSIST_LOGITS  plane r is a handle's M: p = tg_exp(M[c][v] - rshift_r[c]) * rinvz_r[c] -- the expression
//                                             of tg_softmax_out and tg_row_topk, i.e. the bits tg_mapper_result writes;
//                          TG_CONSIST_VEC     plain float planes, every row start 16-byte aligned: 16-byte loads (a quad that
//                                             crosses n_cols is read element by element: nothing behind n_cols is touched);
//                          TG_CONSIST_SCALAR  plain float planes of any pitch and alignment: the same four elements per thread,
//                                             one load each.
//                        Per row:
//                          votes        per plane the column of its largest p, ties to the LOWER column (np.argmax), as spot_offset + v;
//                          vote entropy -sum_s (n_s / R) log(n_s / R) / log(n_cols) over the distinct voted columns s (n_s votes each);
//                          consensus entropy  -sum_v m_v log m_v / log(n_cols), m_v = (p_0v + ... + p_(R-1)v) / R in fp32; a term whose
//                                       m is zero or denormal (< 1.2e-38, a term below 1e-36) counts as 0 -- the hardware logarithm
//                                       takes a denormal for zero, and 0 * -inf must not enter the sum.  The terms are fp32
//                                       (tg_log), their sum is carried in fp64 with the moments;
//                          moments      x_r = (double)p_r - shift (shift = 1 / n_cols: the mean of a softmax row, so the sums stay
//                                       small; the correlation does not depend on it): sum_v x_r per plane and sum_v x_a x_b per pair
//                                       a <= b, every product (fma) and every sum in fp64, carried in registers over ALL rows of the
//                                       workgroup and reduced once -> mom[j][workgroup], j < R + R (R + 1) / 2: first the R sums,
//                                       then the pairs (0,0), (0,1) .. (0,R-1), (1,1), (1,2) ...  (One partial set per workgroup, not
//                                       per row: at 30 000 rows the finish kernel, one workgroup, reads 2 048 x 9 doubles instead of
//                                       30 000 x 9, and a row costs R + 1 wave reductions instead of R + 1 + the moments'.)
//                                       Formed only where a correlation is asked for (mom != null; a uniform branch).
//   tg_consist_finish    ONE workgroup: every moment summed over the workgroups' partials in fp64 (per-thread stride, then a tree), then
//                        r_ab = cov_ab / sqrt(var_a var_b), cov_ab = S_ab - S_a S_b / N, N = n_rows n_cols, for the pairs in the
//                        order of np.tril_indices(R, -1): (1,0), (2,0), (2,1), (3,0) ...  A plane of zero variance gives 0 / 0.
//
//   tg_consist_rows<R, MODE, true> / tg_consist_merge<R>   the same over spot shards: a packet per rank, merged in rank order (at the
//                        end of this file).
//
// Shape of tg_consist_rows (that of tg_row_topk): the row is taken in chunks of TG_CONSIST_CHUNK columns that live in registers, all
// R x TG_CONSIST_NQ loads of a chunk issued before the first use, non-temporal, each element read once.  R is a template argument
// (1 .. TG_CONSIST_MAX_RUNS): the loaded quads, the argmax keys and the R + R (R + 1) / 2 + 1 double accumulators (45 at R = 8) are
// register arrays indexed by unrolled loops only.  The argmax works on the computed p, not on M (two logits can round to one p): a
// float orders like the key of tg_consist_key, a thread meets its columns in ascending order and keeps the first largest, threads and
// waves compare the 64-bit word {key, ~v}.  Columns n_cols .. ld - 1 enter nothing: key 0, p = 0, x = 0.
// Reductions: butterfly inside the wave (all lanes end with the same bits), the four waves through LDS in wave order -- a fixed
// order, no atomics: the same inputs give the same bits on every call.
#pragma once
#include "tg_device.h"

#define TG_CONSIST_MAX_RUNS 8
#define TG_CONSIST_NQ 2                                 // float4 per thread, plane and chunk
#define TG_CONSIST_CHUNK 2048                           // columns per chunk
#define TG_CONSIST_MAX_PARTS 2048                       // workgroups of tg_consist_rows (8 per CU), each one partial set of moments
static_assert(TG_CONSIST_CHUNK == 256 * 4 * TG_CONSIST_NQ, "a chunk is TG_CONSIST_NQ float4 of each of the 256 threads");
enum { TG_CONSIST_LOGITS = 0, TG_CONSIST_VEC = 1, TG_CONSIST_SCALAR = 2 };

TG_HD int tg_consist_nmom(int R) { return R + R * (R + 1) / 2; }
TG_HD int tg_consist_pair(int R, int a, int b) { return R + a * R - a * (a - 1) / 2 + (b - a); }      // moment index of the pair a <= b
// workgroups of tg_consist_rows = partial moment sets: one per row up to TG_CONSIST_MAX_PARTS, then workgroup b takes the rows b, b + parts ...
// (max_parts below TG_CONSIST_MAX_PARTS: the tests' entry point tg_debug_planes_consistency, which walks the row loop with a handful of rows)
TG_HD long long tg_consist_parts(long long n_rows, long long max_parts = TG_CONSIST_MAX_PARTS) { return n_rows < max_parts ? n_rows : max_parts; }
TG_HD size_t tg_consist_bytes(int R, long long n_rows) { return ((size_t)tg_consist_nmom(R) * (size_t)tg_consist_parts(n_rows) * 8 + 255) / 256 * 256; }
// dynamic LDS of tg_consist_rows: [4 waves][moments] doubles, [2][4] entropy sums, [2][4][R] argmax words
TG_HD size_t tg_consist_rows_lds(int R) { return 8 * (size_t)(4 * tg_consist_nmom(R) + 8 + 8 * R); }
#define TG_CONSIST_FINISH_LDS (8 * (256 + TG_CONSIST_MAX_RUNS + TG_CONSIST_MAX_RUNS * (TG_CONSIST_MAX_RUNS + 1) / 2))

struct TgConsistArgs {
    const float* plane[TG_CONSIST_MAX_RUNS];
    const float* rshift[TG_CONSIST_MAX_RUNS];           // (TG_CONSIST_LOGITS only)
    const float* rinvz[TG_CONSIST_MAX_RUNS];
    long long ld;
    int n_cols, n_rows, spot_offset;
    float inv_log_cols;                                 // 1 / ln(n_cols)
    double shift;                                       // 1 / n_cols
    double* mom;                                        // [R + R (R + 1) / 2][workgroups], or null: no correlation is asked for, no moment is formed
    float* vote_ent;                                    // [n_rows] or null
    float* cons_ent;                                    // [n_rows] or null
    int* votes;                                         // [R][n_rows] or null
    // shard form (tg_consist_rows<R, MODE, true>): n_cols are the LOCAL columns, spot_offset the global index of column 0; shift and
    // inv_log_cols are those of the TOTAL number of columns; nothing finished is written, vote_ent / cons_ent / votes are not read
    unsigned long long* words;                          // [R][n_rows] argmax words {key(p), ~global column}, or null
    double* row_cons;                                   // [n_rows] sum_v m_v log m_v over the local columns, or null
};

// a float as an unsigned that orders like it; -0 as +0; >= 1 (0 is "no column")
TG_DEV unsigned tg_consist_key(float p) {
    unsigned u = __builtin_bit_cast(unsigned, p);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the thread's quad at column v < V of a row
template <int MODE> TG_DEV f32x4 tg_consist_load(const float* row, int v, int V) {
    if (MODE == TG_CONSIST_LOGITS || (MODE == TG_CONSIST_VEC && v + 3 < V))       // (logits: the pitch is a multiple of 64, the quad lies inside the row)
        return tg_ld_stream<true>((const f32x4*)(row + v));
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (v + e < V) x[e] = tg_ld_stream<true>(row + v + e);
    return x;
}

TG_DEV unsigned tg_consist_bfly_u(unsigned x, int mask) { return __builtin_bit_cast(unsigned, tg_bfly(__builtin_bit_cast(float, x), mask)); }
// all-reduce over the wave (steps 1, 2, 4 .. 32, as tg_bfly wants them): every lane ends with the same bits
TG_DEV double tg_consist_wave_sum(double x) {
#pragma unroll
    for (int m = 1; m <= 32; m <<= 1) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
        const unsigned lo = tg_consist_bfly_u((unsigned)u, m), hi = tg_consist_bfly_u((unsigned)(u >> 32), m);
        x += __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
    }
    return x;
}
TG_DEV unsigned long long tg_consist_wave_max(unsigned long long w) {
#pragma unroll
    for (int m = 1; m <= 32; m <<= 1) {
        const unsigned lo = tg_consist_bfly_u((unsigned)w, m), hi = tg_consist_bfly_u((unsigned)(w >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        w = o > w ? o : w;
    }
    return w;
}

static inline TgShape tg_consist_rows_shape(long long n_parts, int R) { return tg_shape(n_parts, 1, 256, tg_consist_rows_lds(R)); }

template <int R, int MODE, bool SHARD = false> TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_consist_rows(TgConsistArgs a) {
    TG_LDS_DECL;
    constexpr int NM = R + R * (R + 1) / 2;
    double* wsum = (double*)tg_lds;                                     // [4][NM] the workgroup's moments, once
    double* went = wsum + 4 * NM;                                       // [2][4] entropy sum of a row  } two copies, by row parity: ONE barrier
    unsigned long long* wkey = (unsigned long long*)(went + 8);         // [2][4][R] argmax words       } per row is enough
    const int t = threadIdx.x, V = a.n_cols, lane = t & 63, wave = t >> 6;
    double acc[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) acc[j] = 0.0;
    const double shift = a.shift;
    const bool want_mom = a.mom != nullptr;                             // (uniform: the same for every thread of the grid)
    const float inv_r = 1.f / (float)R;
    int phase = 0;
    for (int c = blockIdx.x; c < a.n_rows; c += gridDim.x, phase ^= 1) {
        const float* row[R];
        float sh[R], iz[R];
        unsigned bk[R];
        int bv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            row[r] = a.plane[r] + (size_t)c * a.ld;
            sh[r] = MODE == TG_CONSIST_LOGITS ? a.rshift[r][c] : 0.f;
            iz[r] = MODE == TG_CONSIST_LOGITS ? a.rinvz[r][c] : 1.f;
            bk[r] = 0u; bv[r] = 0;
        }
        double ent = 0.0;
        for (int v0 = 0; v0 < V; v0 += TG_CONSIST_CHUNK) {
            // ---- the chunk: thread t holds the columns v0 + 4 (256 j + t) + e, e < 4, j < NQ, of every plane
            f32x4 x[R][TG_CONSIST_NQ];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < TG_CONSIST_NQ; ++j) {
                    const int v = v0 + 4 * (256 * j + t);
                    x[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (v < V) x[r][j] = tg_consist_load<MODE>(row[r], v, V);
                }
#pragma unroll
            for (int j = 0; j < TG_CONSIST_NQ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int v = v0 + 4 * (256 * j + t) + e;
                    const bool valid = v < V;
                    float msum = 0.f;
                    float pv[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        float p = x[r][j][e];
                        if (MODE == TG_CONSIST_LOGITS) p = tg_exp(p - sh[r]) * iz[r];
                        p = valid ? p : 0.f;
                        const unsigned k = valid ? tg_consist_key(p) : 0u;
                        if (k > bk[r]) { bk[r] = k; bv[r] = v; }        // (ascending v: the first largest stays)
                        msum += p;
                        pv[r] = p;
                    }
                    if (want_mom) {
                        double dx[R];
#pragma unroll
                        for (int r = 0; r < R; ++r) dx[r] = valid ? (double)pv[r] - shift : 0.0;
                        int q = R;
#pragma unroll
                        for (int g = 0; g < R; ++g) {
                            acc[g] += dx[g];
#pragma unroll
                            for (int h = g; h < R; ++h) { acc[q] = __builtin_fma(dx[g], dx[h], acc[q]); ++q; }
                        }
                    }
                    const float m = msum * inv_r;
                    if (m >= 1.17549435e-38f) ent += (double)(m * tg_log(m));
                }
        }
        // ---- the row's entropy sum and argmax words: wave butterflies, then the four waves in order
        double* ment = went + 4 * phase;
        unsigned long long* mkey = wkey + 4 * R * phase;
        ent = tg_consist_wave_sum(ent);
        if (lane == 0) ment[wave] = ent;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned long long w = tg_consist_wave_max(((unsigned long long)bk[r] << 32) | (unsigned long long)(~(unsigned)bv[r]));
            if (lane == 0) mkey[wave * R + r] = w;
        }
        __syncthreads();
        if (SHARD) {
            // ---- shard form: the row's R words with the GLOBAL column behind the key, and its consensus sum as it stands
            if (t == 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    unsigned long long w = mkey[r];
#pragma unroll
                    for (int u = 1; u < 4; ++u) { const unsigned long long o = mkey[u * R + r]; w = o > w ? o : w; }
                    const unsigned gv = (unsigned)a.spot_offset + ~(unsigned)w;
                    if (a.words) a.words[(size_t)r * a.n_rows + c] = (w & 0xffffffff00000000ull) | (unsigned long long)(~gv);
                }
                if (a.row_cons) a.row_cons[c] = ((ment[0] + ment[1]) + ment[2]) + ment[3];
            }
            continue;
        }
        if (t == 0) {
            int vote[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                unsigned long long w = mkey[r];
#pragma unroll
                for (int u = 1; u < 4; ++u) { const unsigned long long o = mkey[u * R + r]; w = o > w ? o : w; }
                vote[r] = (int)~(unsigned)w;
                if (a.votes) a.votes[(size_t)r * a.n_rows + c] = a.spot_offset + vote[r];
            }
            if (a.cons_ent) a.cons_ent[c] = -(float)(((ment[0] + ment[1]) + ment[2]) + ment[3]) * a.inv_log_cols;
            if (a.vote_ent) {
                float ve = 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    int n = 0;
                    bool first = true;
#pragma unroll
                    for (int u = 0; u < R; ++u)
                        if (vote[u] == vote[r]) { ++n; if (u < r) first = false; }
                    if (first) { const float f = (float)n / (float)R; ve -= f * tg_log(f); }
                }
                a.vote_ent[c] = ve * a.inv_log_cols;
            }
        }
    }
    // ---- the workgroup's moments over all its rows
    if (!want_mom) return;
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const double s = tg_consist_wave_sum(acc[j]);
        if (lane == 0) wsum[wave * NM + j] = s;
    }
    __syncthreads();
    if (t < NM) a.mom[(size_t)t * gridDim.x + blockIdx.x] = ((wsum[t] + wsum[NM + t]) + wsum[2 * NM + t]) + wsum[3 * NM + t];
}

// mom [nm][n_parts] -> pearson [R (R - 1) / 2] (or null) and / or the sums themselves, sums [nm] (or null: the shard form asks for them);
// one workgroup of 256 threads
TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_consist_finish(const double* mom, int n_parts, int R, double n_elem, double* pearson, double* sums) {
    TG_LDS_DECL;
    double* red = (double*)tg_lds;                                      // [256]
    double* fin = red + 256;                                            // [nm]
    const int t = threadIdx.x, nm = tg_consist_nmom(R);
    for (int j = 0; j < nm; ++j) {
        const double* col = mom + (size_t)j * n_parts;
        double s = 0.0;
        for (int i = t; i < n_parts; i += 256) s += col[i];             // (at most TG_CONSIST_MAX_PARTS / 256 = 8 trips)
        red[t] = s;
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) fin[j] = red[0];
        __syncthreads();
    }
    if (sums && t < nm) sums[t] = fin[t];                               // shard form: the local sums, no correlation
    if (pearson && t < R * (R - 1) / 2) {
        int g = 1;                                                      // pair t of np.tril_indices(R, -1): (g, h), g > h
        while (g * (g + 1) / 2 <= t) ++g;
        const int h = t - g * (g - 1) / 2;
        const double sg = fin[g], sh = fin[h];
        const double cov = fin[tg_consist_pair(R, h, g)] - sg * sh / n_elem;
        const double vg = fin[tg_consist_pair(R, g, g)] - sg * sg / n_elem, vh = fin[tg_consist_pair(R, h, h)] - sh * sh / n_elem;
        pearson[t] = cov / sqrt(vg * vh);
    }
}

// ---- spot shards ------------------------------------------------------------------------------------------------------------------
// Every rank holds a block of the columns.  tg_consist_rows<R, MODE, true> + tg_consist_finish(sums) leave a PACKET of 8-byte units,
//   [nm moment sums][n_rows consensus sums][R][n_rows] argmax words        (tg_consist_packet_units; n_rows = 0: the moments alone)
// with shift and the entropies' divisor taken from the TOTAL number of columns and the global column behind every key.  The W packets
// are gathered in rank order, and tg_consist_merge<R> answers on every rank, everything in ascending rank order:
//   votes              the maximum of the ranks' words: equal p on two ranks goes to the lower global column
//   vote entropy       from the merged votes, as tg_consist_rows forms it
//   consensus entropy  -(float)(rank-order fp64 sum of the consensus sums) * 1 / ln(total columns)
//   pearson            from the rank-order sums of the moments with N = n_elem, pairs in np.tril_indices(R, -1) order (workgroup 0)
// A thread per row; R is a template argument: the votes live in registers.
TG_HD size_t tg_consist_packet_units(int R, long long n_rows) { return (size_t)tg_consist_nmom(R) + (size_t)n_rows * (size_t)(1 + R); }

struct TgConsistMergeArgs {
    const unsigned long long* packets;                  // [W][stride] 8-byte units
    long long stride;
    int n_ranks, n_rows;
    float inv_log_cols;                                 // 1 / ln(total columns)
    double n_elem;                                      // elements of a whole plane
    double* pearson;                                    // [R (R - 1) / 2] or null
    float* vote_ent;                                    // [n_rows] or null
    float* cons_ent;                                    // [n_rows] or null
    int* votes;                                         // [R][n_rows] or null
};

static inline TgShape tg_consist_merge_shape(long long n_rows) { return tg_shape(n_rows > 0 ? (n_rows + 255) / 256 : 1, 1, 256, 0); }

TG_DEV double tg_consist_rank_sum(const TgConsistMergeArgs& a, size_t unit) {
    const double* p = (const double*)a.packets + unit;
    double s = p[0];
    for (int w = 1; w < a.n_ranks; ++w) s += p[(size_t)w * (size_t)a.stride];      // ascending ranks
    return s;
}

template <int R> TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_consist_merge(TgConsistMergeArgs a) {
    constexpr int NM = R + R * (R + 1) / 2;
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && a.pearson && t < R * (R - 1) / 2) {
        int g = 1;                                                      // pair t of np.tril_indices(R, -1): (g, h), g > h
        while (g * (g + 1) / 2 <= t) ++g;
        const int h = t - g * (g - 1) / 2;
        const double sg = tg_consist_rank_sum(a, g), sh = tg_consist_rank_sum(a, h);
        const double cov = tg_consist_rank_sum(a, tg_consist_pair(R, h, g)) - sg * sh / a.n_elem;
        const double vg = tg_consist_rank_sum(a, tg_consist_pair(R, g, g)) - sg * sg / a.n_elem;
        const double vh = tg_consist_rank_sum(a, tg_consist_pair(R, h, h)) - sh * sh / a.n_elem;
        a.pearson[t] = cov / sqrt(vg * vh);
    }
    const long long c = (long long)blockIdx.x * 256 + t;
    if (c >= a.n_rows) return;
    if (a.cons_ent) a.cons_ent[c] = -(float)tg_consist_rank_sum(a, (size_t)NM + (size_t)c) * a.inv_log_cols;
    if (!a.votes && !a.vote_ent) return;
    int vote[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned long long* p = a.packets + (size_t)NM + (size_t)a.n_rows * (size_t)(1 + r) + (size_t)c;
        unsigned long long w = p[0];
        for (int k = 1; k < a.n_ranks; ++k) { const unsigned long long o = p[(size_t)k * (size_t)a.stride]; w = o > w ? o : w; }
        vote[r] = (int)~(unsigned)w;
        if (a.votes) a.votes[(size_t)r * a.n_rows + c] = vote[r];
    }
    if (a.vote_ent) {
        float ve = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int n = 0;
            bool first = true;
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (vote[u] == vote[r]) { ++n; if (u < r) first = false; }
            if (first) { const float f = (float)n / (float)R; ve -= f * tg_log(f); }
        }
        a.vote_ent[c] = ve * a.inv_log_cols;
    }
}

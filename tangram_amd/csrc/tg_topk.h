// tg_topk.h -- each cell's k most probable spots straight from the logits: C x k (value, spot) pairs instead of the dense C x V plane
// that tg_softmax_out writes (1.2 GB at 30 000 x 10 000, 40 GB at 200 000 x 50 000).
//
//   tg_row_topk          one 256-thread workgroup per row of M: the k largest p[c][v] = tg_exp(M[c][v] - rshift[c]) * rinvz[c] -- the
//                        expression of tg_softmax_out, so the values are the bits tg_mapper_result writes -- with their GLOBAL spot
//                        indices (spot_offset + v).  Order: value descending, equal values by ascending spot.  1 <= k <= TG_TOPK_MAX.
//   tg_topk_merge_rows   merges per-row candidate lists [n_rows][n_in] of (value, index) into the best k under the same order (the
//                        lists of the spot shards of one row); index -1 marks a pad, which sorts after every real entry.
//
// Selection and order work on the computed p, never on M (two logits can round to the same p): a non-negative float orders like its
// bit pattern, so an entry is the 64-bit word {bits(p) + 1, ~v} -- larger word = earlier in the result, and no two entries of a row
// are equal (0 in the high half is kept for "no element": padding columns V .. Vp - 1 get it and can never be selected).
//
// Shape of tg_row_topk, and why not the LDS-staged radix select: the row is taken in chunks of TG_TOPK_CHUNK = 8 192 spots that
// live in REGISTERS (8 float4 per thread, all loads of a chunk issued before the first use: 32 KB in flight per workgroup, each
// logit read from HBM once, non-temporally).  A radix select over a row staged in LDS builds its histograms with LDS atomics, and
// the keys of a softmax row share their leading byte (every p of a row lies within a few binades): the first passes would put
// thousands of adds on one or two counters, one LDS cycle each, and 40 - 64 KB of LDS per workgroup would leave 2 - 4 workgroups
// per CU to hide HBM latency.  Here LDS holds 6 KB and the occupancy is set by the registers.  Per chunk:
//   1. every thread takes the maximum of its 32 keys, pairs of threads (t, t + 128) the larger of theirs; T = the k-th largest of
//      these 128 maxima (threads 0 - 127 rank one each against the others, broadcast reads).  k different elements >= T exist, so
//      the k-th largest key of the chunk is >= T: only keys >= T can be selected -- a few more than k of them on a row without
//      structure (k = 64: T is the median of the 128 maxima, about 1 % of the chunk survives).  From the second chunk on also > the
//      k-th key carried so far (an equal key of a later chunk has a larger spot index and loses).
//      (Ranking all 256 thread maxima, four times the compares, measured 1.12 ms at 30 000 x 10 000, k = 8; this form 0.57 ms,
//      tg_softmax_out 0.52 ms in the same run: what the kernel costs over the read is this step, not the list or its ordering.)
//   2. the survivors are appended to a candidate list in LDS behind the carried entries (one LDS atomic add per thread that has
//      any).  More than TG_TOPK_CAP of them (rows of equal logits, maxima that all sit in few threads): the exact k-th key is found
//      by bisection on the key bits (31 block-wide counts over the registers), then the ties at that key that still fit by
//      bisection on the position inside the chunk (13 counts); exactly k elements are appended.
//   3. every candidate counts the candidates that precede it: that count IS its place, the first k are the new carry.
// No global atomics, no polling, nothing of the handle's workspace is written.
#pragma once
#include "tg_device.h"

#define TG_TOPK_MAX 64
#define TG_TOPK_NQ 8                                    // float4 per thread and chunk
#define TG_TOPK_CHUNK (256 * 4 * TG_TOPK_NQ)            // spots per chunk
#define TG_TOPK_CAP 448                                 // candidates of one chunk the list takes (+ TG_TOPK_MAX carried = 512 entries)
#define TG_TOPK_CHUNK_BITS 13
static_assert((1 << TG_TOPK_CHUNK_BITS) == TG_TOPK_CHUNK, "TG_TOPK_CHUNK_BITS is log2 of the chunk");
#define TG_MERGE_CHUNK 512                              // entries of an input list ranked at a time by tg_topk_merge_rows
#define TG_TOPK_LDS (8 * (TG_TOPK_MAX + TG_MERGE_CHUNK) + 8 * TG_TOPK_MAX + 4 * 256 + 64)

typedef unsigned long long tg_u64;

TG_DEV int tg_topk_shfl_xor(int v, int mask) { return __builtin_bit_cast(int, tg_shfl_xor(__builtin_bit_cast(float, v), mask)); }

// sum of x over the 256 threads; `red`: 8 ints of LDS, `phase` alternates between its halves so that ONE barrier per call is enough
// (a thread can be at most one call ahead of the slowest one)
TG_DEV int tg_topk_block_sum(int x, int* red, int& phase) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += tg_topk_shfl_xor(x, m);
    int* slot = red + 4 * (phase & 1);
    ++phase;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = x;
    __syncthreads();
    return slot[0] + slot[1] + slot[2] + slot[3];
}

// list[0 .. n) -> its best k entries, in order, in list[0 .. k) (0 = pad: behind every entry, as many as k - #entries).
// The entries of a list are pairwise different, so "how many are larger than mine" is the place of an entry.
TG_DEV void tg_topk_rank_keep(tg_u64* list, int n, int k, tg_u64* keep) {
    const int t = threadIdx.x;
    if (t < TG_TOPK_MAX) keep[t] = 0ull;
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const tg_u64 mine = list[i];
        if (mine == 0ull) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) r += list[j] > mine ? 1 : 0;
        if (r < k) keep[r] = mine;
    }
    __syncthreads();
    if (t < k) list[t] = keep[t];
    __syncthreads();
}

struct TgTopkArgs {
    const float *M, *rshift, *rinvz;
    int V, Vp, k, spot_offset;
    float* val;       // [C][k]
    int* idx;         // [C][k]
};

// is element `key` at position `pos` of the chunk selected?  key > above, or key == above at a position <= tie_pos
TG_DEV bool tg_topk_pick(unsigned key, int pos, unsigned above, int tie_pos) { return key > above || (key == above && pos <= tie_pos); }

TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_row_topk(TgTopkArgs a) {
    TG_LDS_DECL;
    tg_u64* list = (tg_u64*)tg_lds;                                     // [TG_TOPK_MAX carried + TG_TOPK_CAP of this chunk]
    tg_u64* keep = list + TG_TOPK_MAX + TG_MERGE_CHUNK;                 // [TG_TOPK_MAX]
    unsigned* tmax = (unsigned*)(keep + TG_TOPK_MAX);                   // [256]
    int* red = (int*)(tmax + 256);                                      // [8] block sums
    int* ctr = red + 8;                                                 // [0] list cursor, [1] T
    const int c = blockIdx.x, t = threadIdx.x, k = a.k, V = a.V;
    const float* row = a.M + (size_t)c * a.Vp;
    const float sh = a.rshift[c], iz = a.rinvz[c];
    int ncarry = 0, phase = 0;
    if (t == 0) ctr[0] = 0;
    for (int v0 = 0; v0 < V; v0 += TG_TOPK_CHUNK) {
        // ---- the chunk: thread t holds the spots v0 + 4 (256 j + t) + e, e < 4, j < NQ; key 0 = no spot
        unsigned key[4 * TG_TOPK_NQ];
        f32x4 x[TG_TOPK_NQ];
#pragma unroll
        for (int j = 0; j < TG_TOPK_NQ; ++j) {
            const int v = v0 + 4 * (256 * j + t);
            x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (v < V) x[j] = tg_ld_stream<true>((const f32x4*)(row + v));        // (Vp is a multiple of 64: the quad lies inside the row)
        }
        unsigned mx = 0;
#pragma unroll
        for (int j = 0; j < TG_TOPK_NQ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + 4 * (256 * j + t) + e;
                const float p = tg_exp(x[j][e] - sh) * iz;
                const unsigned kk = v < V ? __builtin_bit_cast(unsigned, p) + 1u : 0u;
                key[4 * j + e] = kk;
                mx = kk > mx ? kk : mx;
            }
        // ---- 1. T = k-th largest of the 128 maxima of thread pairs (t, t + 128); threads 0 - 127 rank one each
        if (t >= 128) tmax[t] = mx;
        __syncthreads();
        if (t < 128) { const unsigned o = tmax[t + 128]; mx = o > mx ? o : mx; tmax[t] = mx; }
        __syncthreads();
        if (t < 128) {
            int r = 0;
#pragma unroll 2
            for (int s = 0; s < 128; s += 4) {
                const u32x4 o = *(const u32x4*)(tmax + s);
#pragma unroll
                for (int e = 0; e < 4; ++e) r += (o[e] > mx || (o[e] == mx && s + e < t)) ? 1 : 0;
            }
            if (r == k - 1) ctr[1] = (int)mx;
        }
        __syncthreads();
        unsigned T = (unsigned)ctr[1];
        if (T < 1u) T = 1u;
        if (ncarry == k) {                                   // the carry is full: only keys above its last entry can enter
            const unsigned last = (unsigned)(list[k - 1] >> 32);
            if (last + 1u > T) T = last + 1u;
        }
        unsigned above = T - 1u;
        int tie_pos = -1;
        // ---- 2. the survivors behind the carry
        for (int attempt = 0; attempt < 2; ++attempt) {
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < 4 * TG_TOPK_NQ; ++i) cnt += tg_topk_pick(key[i], 4 * (256 * (i >> 2) + t) + (i & 3), above, tie_pos) ? 1 : 0;
            int at = cnt ? tg_lds_atomic_add(ctr, cnt) : 0;
            if (cnt && at + cnt <= TG_TOPK_CAP) {
#pragma unroll
                for (int i = 0; i < 4 * TG_TOPK_NQ; ++i) {
                    const int pos = 4 * (256 * (i >> 2) + t) + (i & 3);
                    if (tg_topk_pick(key[i], pos, above, tie_pos))
                        list[ncarry + at++] = ((tg_u64)key[i] << 32) | (tg_u64)(~(unsigned)(v0 + pos));
                }
            }
            __syncthreads();
            const int total = ctr[0];
            __syncthreads();
            if (t == 0) ctr[0] = 0;
            if (total <= TG_TOPK_CAP) { ncarry += total; break; }
            // more than the list takes: the exact k-th key by bisection (count(key >= X) >= k holds for X = 1: total > CAP >= k) ...
            unsigned X = 0;
            for (int b = 30; b >= 0; --b) {
                const unsigned cand = X | (1u << b);
                int n = 0;
#pragma unroll
                for (int i = 0; i < 4 * TG_TOPK_NQ; ++i) n += key[i] >= cand ? 1 : 0;
                if (tg_topk_block_sum(n, red, phase) >= k) X = cand;
            }
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4 * TG_TOPK_NQ; ++i) n += key[i] > X ? 1 : 0;
            const int need = k - tg_topk_block_sum(n, red, phase);          // >= 1 ties at X to take, lowest positions first
            // ... and the position of the need-th tie: the largest Y with fewer than `need` ties in front of it
            int Y = 0;
            for (int b = TG_TOPK_CHUNK_BITS - 1; b >= 0; --b) {
                const int cand = Y | (1 << b);
                int m = 0;
#pragma unroll
                for (int i = 0; i < 4 * TG_TOPK_NQ; ++i) m += (key[i] == X && 4 * (256 * (i >> 2) + t) + (i & 3) < cand) ? 1 : 0;
                if (tg_topk_block_sum(m, red, phase) < need) Y = cand;
            }
            above = X; tie_pos = Y;                          // exactly k elements now (the barrier of the last sum orders ctr[0] = 0)
        }
        // ---- 3. order the list, keep the first k
        tg_topk_rank_keep(list, ncarry, k, keep);
        ncarry = ncarry < k ? ncarry : k;
    }
    for (int r = t; r < k; r += 256) {
        const tg_u64 e = r < ncarry ? list[r] : 0ull;
        const bool real = e != 0ull;
        a.val[(size_t)c * k + r] = real ? __builtin_bit_cast(float, (unsigned)(e >> 32) - 1u) : 0.f;
        a.idx[(size_t)c * k + r] = real ? a.spot_offset + (int)~(unsigned)e : -1;
    }
}

// a float as an unsigned that orders like it (>= 1 for every value but the all-ones NaN)
TG_DEV unsigned tg_topk_okey(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
TG_DEV float tg_topk_okey_inv(unsigned o) { return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// One workgroup per row.  The indices of a row's real entries must be pairwise different (they are spots of different shards).
// An entry here is {okey(value), ~index << 1 | sign bit of a zero}: -0.0 takes the key of +0.0 -- the two are equal as floats, so the
// lower spot index decides between them like between any equal values -- and its sign bit travels in the bit that ~index leaves free
// (an index is below 2^31: the top bit of ~index is always set and need not be stored); the indices differ, so it never decides an order.
TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_topk_merge_rows(const float* val_in, const int* idx_in, int n_in, long long ld_in, int k,
                                                        float* val_out, int* idx_out) {
    TG_LDS_DECL;
    tg_u64* list = (tg_u64*)tg_lds;                                     // [TG_TOPK_MAX carried + TG_MERGE_CHUNK]
    tg_u64* keep = list + TG_TOPK_MAX + TG_MERGE_CHUNK;
    const int t = threadIdx.x;
    const size_t row = (size_t)blockIdx.x;
    int ncarry = 0;
    for (int j0 = 0; j0 < n_in; j0 += TG_MERGE_CHUNK) {
        const int n = n_in - j0 < TG_MERGE_CHUNK ? n_in - j0 : TG_MERGE_CHUNK;
        for (int i = t; i < n; i += 256) {
            const float v = val_in[row * ld_in + j0 + i];
            const int ix = idx_in[row * ld_in + j0 + i];
            const bool negzero = __builtin_bit_cast(unsigned, v) == 0x80000000u;
            list[ncarry + i] = ix < 0 ? 0ull                                                                    // a pad: behind everything
                                      : (((tg_u64)tg_topk_okey(negzero ? 0.f : v) << 32) | (tg_u64)((~(unsigned)ix << 1) | (negzero ? 1u : 0u)));
        }
        __syncthreads();
        tg_topk_rank_keep(list, ncarry + n, k, keep);
        ncarry = k;
    }
    for (int r = t; r < k; r += 256) {
        const tg_u64 e = list[r];
        const bool real = e != 0ull;
        val_out[row * k + r] = real ? (((unsigned)e & 1u) ? -0.f : tg_topk_okey_inv((unsigned)(e >> 32))) : 0.f;
        idx_out[row * k + r] = real ? (int)~(((unsigned)e >> 1) | 0x80000000u) : -1;
    }
}

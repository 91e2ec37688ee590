// tg_sparse.h -- project genes from a SPARSE mapping: out[V][n_genes] = X^T S for a canonical CSR X [C][V] with a few entries per
// row (each cell's k most probable spots, tg_topk.h) and a dense S [C][n_genes].  At k = 8 and 10 000 spots X is 0.08 % dense: no
// matrix core applies, the product is a gather of rows of S per spot, bound by memory traffic.  Algorithmic bytes:
// 4 nnz n_genes of gathered S rows + 4 V n_genes written.
//
// Two steps, both without float atomics, both bit-reproducible:
//
//   1. the SPOT-MAJOR IMAGE of X (tg_sparse_map_build): spot_ptr int64 [V + 1], cell int32 [nnz], val float [nnz] -- the entries of
//      spot v are cell[spot_ptr[v] .. spot_ptr[v + 1]), ORDERED BY ASCENDING CELL INDEX.  CSR is canonical (a spot holds a cell at
//      most once), so this order is unique and the image a pure function of X.
//        tg_sp_count     one thread per entry: an INTEGER atomic add on its spot's counter (counts do not depend on order)
//        tg_sp_scan      one workgroup: exclusive prefix sum of the V counts -> spot_ptr; the counters are cleared for reuse
//        tg_sp_scatter   one thread per entry: its row by bisection of indptr, its slot spot_ptr[v] + (atomic cursor of v) in a
//                        STAGING copy of the image -- complete, but in arrival order inside a spot
//        tg_sp_order     one workgroup per spot: every entry counts the entries of its spot with a smaller cell index -- that count
//                        IS its place -- and is written there, out of place (staging -> image).  The cell indices are ranked from
//                        LDS, TG_SP_TILE at a time, so a spot that holds every cell (longer than a workgroup, than a tile) works
//                        like any other; it costs n^2 / 256 LDS reads per thread, nothing anyone waits for at a few entries per spot.
//   2. the projection (tg_sp_project): one workgroup per (spot, tile of 1 024 genes); threads take adjacent genes, so every S row
//      segment is read coalesced; out[v][g] = one fmaf chain from 0 over the entries of v IN THE IMAGE'S ORDER.  (c, p) are uniform
//      over the workgroup.  TG_SP_AHEAD entries' row loads are issued before the first fma of the batch: without that the loop pays
//      one memory latency per entry.  <VEC>: 16-byte loads and stores (thread t: genes 4 t .. 4 t + 3 of the tile) when the bases are
//      16-byte aligned and the pitches multiples of 4 floats, else scalar ones (genes t + 256 e): each output element is the same
//      chain of the same operands either way.  A spot without entries writes zeros.  Workgroups are ordered tile-major (all spots of
//      gene tile 0, then tile 1, ...): a cell's row segment is wanted by the ~k spots the cell maps to, and one tile's segments of
//      every cell (4 KB x C: 123 MB at 30 000 cells) can stay in the Infinity Cache between those uses.
#pragma once
#include "tg_device.h"

#define TG_SP_TILE 1024                 // cell indices ranked from LDS at a time (tg_sp_order)
#define TG_SP_GENES 1024                // genes per workgroup of tg_sp_project: 256 threads x 4
#define TG_SP_AHEAD 8                   // entries whose S rows are loaded before the first fma of a batch

// byte offsets inside the caller's workspace (every array 256-byte aligned); the first three are the image
struct TgSparseMapLayout { size_t o_ptr, o_cell, o_val, o_cnt, o_tcell, o_tval, bytes; };
TG_HD TgSparseMapLayout tg_sparse_map_layout(long long n_spots, long long nnz) {
    TgSparseMapLayout L;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t o = at; at += (n + 255) / 256 * 256; return o; };
    L.o_ptr = take(8 * ((size_t)n_spots + 1));
    L.o_cell = take(4 * (size_t)nnz);
    L.o_val = take(4 * (size_t)nnz);
    L.o_cnt = take(4 * (size_t)n_spots);
    L.o_tcell = take(4 * (size_t)nnz);
    L.o_tval = take(4 * (size_t)nnz);
    L.bytes = at ? at : 256;
    return L;
}

TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_sp_count(const int* indices, long long nnz, int* cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nnz) tg_global_atomic_add(cnt + indices[i], 1);
}

// spot_ptr[v] = cnt[0] + ... + cnt[v - 1], spot_ptr[V] = nnz; cnt <- 0 (the cursors of tg_sp_scatter).  ONE workgroup of 1 024
// threads, thread t owns the spots [t chunk, (t + 1) chunk).
TG_KERNEL void TG_LAUNCH_BOUNDS(1024) tg_sp_scan(int* cnt, long long V, long long* spot_ptr) {
    TG_LDS_DECL;
    long long* part = (long long*)tg_lds;                               // [1024]
    const int t = threadIdx.x;
    const long long chunk = (V + 1023) / 1024;
    const long long beg = t * chunk < V ? t * chunk : V, end = beg + chunk < V ? beg + chunk : V;
    long long s = 0;
    for (long long v = beg; v < end; ++v) s += cnt[v];
    part[t] = s;
    __syncthreads();
    long long run = 0;
    for (int j = 0; j < t; ++j) run += part[j];
    for (long long v = beg; v < end; ++v) {
        spot_ptr[v] = run;
        run += cnt[v];
        cnt[v] = 0;
    }
    if (t == 1023) spot_ptr[V] = run;                                   // (its own range ends at V, empty or not)
}

TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_sp_scatter(const long long* indptr, const int* indices, const float* data, int C, long long nnz,
                                                   const long long* spot_ptr, int* cnt, int* tcell, float* tval) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    int lo = 0, hi = C;                                                 // indptr[lo] <= i < indptr[hi] (indptr[0] = 0, indptr[C] = nnz)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (indptr[mid] <= i) lo = mid; else hi = mid;
    }
    const int v = indices[i];
    const long long slot = spot_ptr[v] + tg_global_atomic_add(cnt + v, 1);
    tcell[slot] = lo;
    tval[slot] = data[i];
}

TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_sp_order(const long long* spot_ptr, const int* tcell, const float* tval, int* cell, float* val) {
    TG_LDS_DECL;
    int* tile = (int*)tg_lds;                                           // [TG_SP_TILE]
    const int t = threadIdx.x;
    const long long beg = spot_ptr[blockIdx.x], n = spot_ptr[blockIdx.x + 1] - beg;
    const bool once = n <= TG_SP_TILE;                                  // the whole spot fits the tile: staged once
    for (long long jb = 0; jb < n; jb += 256) {
        const long long j = jb + t;
        const int mine = j < n ? tcell[beg + j] : 0;
        long long r = 0;
        for (long long i0 = 0; i0 < n; i0 += TG_SP_TILE) {
            const int m = (int)(n - i0 < TG_SP_TILE ? n - i0 : TG_SP_TILE);
            if (!once || jb == 0) {
                __syncthreads();                                        // (the previous tile has been read by everybody)
                for (int i = t; i < m; i += 256) tile[i] = tcell[beg + i0 + i];
                __syncthreads();
            }
            if (j < n)
                for (int i = 0; i < m; ++i) r += tile[i] < mine ? 1 : 0;
        }
        if (j < n) {
            cell[beg + r] = mine;
            val[beg + r] = tval[beg + j];
        }
    }
}

struct TgSparseProjArgs {
    const long long* spot_ptr;
    const int* cell;
    const float* val;
    const float* S;
    long long ld_s;
    int n_genes;
    float* out;
    long long ld_out;
    int v0, nv;                         // this launch: the spots [v0, v0 + nv); workgroup b -> gene tile b / nv, spot v0 + b % nv
};

// The thread's four elements of a row whose first one is p[0]: VEC: p[0 .. 3], else p[0], p[256], p[512], p[768]; the elements
// 0 .. last exist.  FULL (VEC, last = 3): one 16-byte access.  Otherwise four scalar loads WITHOUT a branch -- a guard per load would
// put a wait between the loads of a batch --: an element that does not exist re-reads element `last` and is dropped at the store.
template <bool VEC, bool FULL> TG_DEV f32x4 tg_sp_load(const float* p, int last) {
    if constexpr (VEC && FULL) return *(const f32x4*)p;
    constexpr int step = VEC ? 1 : 256;
    f32x4 x;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = p[(e < last ? e : last) * step];
    return x;
}
template <bool VEC, bool FULL> TG_DEV void tg_sp_store(float* p, int last, f32x4 x) {
    if constexpr (VEC && FULL) { __builtin_nontemporal_store(x, (f32x4*)p); return; }
    constexpr int step = VEC ? 1 : 256;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e <= last) __builtin_nontemporal_store(x[e], p + e * step);
}

// the fmaf chains of one thread over the entries [beg, end) of its spot; Sg = S + the thread's first gene
template <bool VEC, bool FULL> TG_DEV f32x4 tg_sp_chain(const TgSparseProjArgs& a, const float* Sg, long long beg, long long end, int last) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    long long e = beg;
    for (; e + TG_SP_AHEAD <= end; e += TG_SP_AHEAD) {
        float p[TG_SP_AHEAD];
        f32x4 x[TG_SP_AHEAD];
#pragma unroll
        for (int u = 0; u < TG_SP_AHEAD; ++u) {
            p[u] = a.val[e + u];
            x[u] = tg_sp_load<VEC, FULL>(Sg + (long long)a.cell[e + u] * a.ld_s, last);
        }
#pragma unroll
        for (int u = 0; u < TG_SP_AHEAD; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(p[u], x[u][k], acc[k]);
    }
    if (e < end) {                      // the last m = 1 .. AHEAD - 1 entries: the same batch; a slot past the end re-reads entry end - 1 (no
        const int m = (int)(end - e);   // branch between the loads) and is left out of the chain
        float p[TG_SP_AHEAD - 1];
        f32x4 x[TG_SP_AHEAD - 1];
#pragma unroll
        for (int u = 0; u < TG_SP_AHEAD - 1; ++u) {
            const long long eu = e + (u < m ? u : m - 1);
            p[u] = a.val[eu];
            x[u] = tg_sp_load<VEC, FULL>(Sg + (long long)a.cell[eu] * a.ld_s, last);
        }
#pragma unroll
        for (int u = 0; u < TG_SP_AHEAD - 1; ++u)
            if (u < m) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(p[u], x[u][k], acc[k]);
            }
    }
    return acc;
}

template <bool VEC> TG_KERNEL void TG_LAUNCH_BOUNDS(256) tg_sp_project(TgSparseProjArgs a) {
    constexpr int step = VEC ? 1 : 256;
    const int v = a.v0 + (int)(blockIdx.x % (unsigned)a.nv);
    const long long g = (long long)(blockIdx.x / (unsigned)a.nv) * TG_SP_GENES + (VEC ? 4 : 1) * (int)threadIdx.x;
    if (g >= a.n_genes) return;                                         // (no barrier below)
    const long long left = (a.n_genes - g + step - 1) / step;           // elements g, g + step, ... below n_genes
    const int last = left < 4 ? (int)left - 1 : 3;
    const long long beg = a.spot_ptr[v], end = a.spot_ptr[v + 1];
    const float* Sg = a.S + g;
    float* og = a.out + (long long)v * a.ld_out + g;
    if (VEC && last == 3) tg_sp_store<VEC, true>(og, last, tg_sp_chain<VEC, true>(a, Sg, beg, end, last));
    else tg_sp_store<VEC, false>(og, last, tg_sp_chain<VEC, false>(a, Sg, beg, end, last));
}

/* CDNA4 (gfx950) aligner core: adaptive-banded sequence-to-graph DP.
 *
 * One alignment job per 512-thread workgroup (8 wavefronts). The block
 * sweeps the graph's topologically-sorted rows; the 8 waves cover a row's
 * band at once, in 512-cell superchunks where the band is wider:
 *   - M/E gather from predecessor rows. Recent rows are kept in LDS — a
 *     ~50-cycle LDS read replaces a ~900-cycle HBM round-trip on the
 *     row-to-row dependent chain: the convex kernel keeps a ring of the last
 *     rows, the affine and linear kernels a double-buffered copy of the
 *     previous row. Other predecessors (and bands wider than BMW cells)
 *     read the banded HBM arena with coalesced 2/4-byte loads;
 *   - the F (insertion) recurrence is a per-wave max-plus scan (DPP row
 *     shifts + readlane carries) plus a cross-wave carry recurrence over
 *     the published wave edges, with a carry between superchunks;
 *   - the banded planes stream to the HBM arena with coalesced stores
 *     (convex: H,E1,E2 only — the F planes are recomputed from stored H at
 *     backtrack time; affine: H,E1,F1; linear: H);
 *   - the row argmax (adaptive band steering) is a per-wave reduction and
 *     an 8-way combine from LDS;
 *   - per-row band metadata is one 16-byte abamd_row_meta_t;
 *   - thread 0 backtracks in the kernel.
 * Integer max-plus throughout: MFMA does not apply; the target bound is the
 * 6 B/cell (convex int16) HBM plane traffic.
 *
 * Three kernels, each instantiated for int16 and for the int32 overflow
 * rescore, each serving global, local and extension mode: cg_global_mw_kernel
 * (convex gaps, the north-star path), ag_global_mw_kernel (affine) and
 * lg_global_mw_kernel (linear). The convex kernel has a second template
 * flag, FAST, for the north-star case (global, banded, no path scores, full
 * ring depth): mode tests folded away, rolled row scalars as batched scalar
 * loads; FAST = false serves everything else. The affine and linear kernels
 * are the "multi-wave frame" section plus their recurrence. The convex kernel keeps its own text (rolled
 * predecessors, row ring, global-address-space pointers): calling the frame
 * for the three blocks it has in common measured 0.5 % lower at the bench
 * (DESIGN.md §6b); small source changes move these kernels' SGPR spills.
 *
 * Numerics are bit-identical to oracle/ref_core.c (and the reference x86
 * build): int16 arithmetic wraps (non-saturating _mm*_add_epi16 semantics),
 * reproduced by truncating to the score type after every add/sub. Recurrence
 * and backtrack follow abpoa_align_simd.c:935-1074 / :309-458; band formulas
 * abpoa_align.h:34-35. The host picks the kernel by gap model and score
 * width (gpu_align.cpp, gpu_batch_resident.cpp).
 */
#include <hip/hip_runtime.h>
#include <type_traits>
#include "gpu_core.h"

/* Compile-time phase profiler (make kprof): accumulates s_memtime cycles per
 * row-loop phase of the convex kernel across all jobs. Diagnostic build
 * only — never part of the product library. */
#ifdef ABAMD_KPROF
/* slots 0..15: phase totals; 16..30: the convex multi-wave kernel's rows by
 * class (0 = one predecessor r-1 in the ring, 1 = all predecessors in the
 * ring, 2 = at least one arena gather): rows 16+c, gather+hpre cycles 19+c,
 * epilogue cycles 22+c, row cycles 25+c; 28 rows wider than a ring slot,
 * 29 rows with more than MW_NPF predecessors, 30 predecessor references */
#define ABAMD_KPROF_N 32
__device__ unsigned long long abamd_kprof_acc[ABAMD_KPROF_N];
extern "C" void abamd_kprof_fetch(unsigned long long *out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(abamd_kprof_acc), sizeof(abamd_kprof_acc));
}
extern "C" void abamd_kprof_reset(void) {
    unsigned long long z[ABAMD_KPROF_N] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(abamd_kprof_acc), z, sizeof(z));
}
#define KPROF_T(v) unsigned long long v = __builtin_readcyclecounter()
#define KPROF_ACC(slot, val) if (lane == 0) atomicAdd(&abamd_kprof_acc[slot], (unsigned long long)(val))
#else
#define KPROF_T(v)
#define KPROF_ACC(slot, val)
#endif

#define WAVE 64
#define MWAVES 8
#define MWT (WAVE * MWAVES)
/* LDS row-cache width (cells): a ring slot of the convex kernel, the
 * previous-row buffer of the affine and linear ones. Default bands are
 * ~230-450 cells (w = wb + wf*qlen = 110 at the north-star shape); wider
 * rows are re-read from the arena. */
#define BMW 512

template <typename S>
__device__ __forceinline__ S smax(S a, S b) { return a > b ? a : b; }

/* Wave-wide inclusive max-plus scan with decay `e` per lane step:
 *   out[l] = max_{k<=l} (in[k] - (l-k)*e)
 * Intra-row (16-lane) steps use DPP row_shr (VALU latency) instead of
 * ds_bpermute; only the two cross-row steps pay the LDS-unit latency.
 * Arithmetic wraps at the score width after every op (reference int16
 * semantics). `neutral` fills lanes with no source. */
template <typename S>
__device__ __forceinline__ S scan_maxplus(S f, int e, S neutral, int lane) {
    (void)neutral;
    /* lanes with no in-row source keep their own value (old = f), exactly
     * like the guarded shuffle formulation — a synthetic floor could exceed
     * the reference's stored out-of-band values and break bit-parity */
    int cand;
    cand = __builtin_amdgcn_update_dpp((int)f, (int)f, 0x111, 0xf, 0xf, false);
    if ((lane & 15) >= 1) f = smax(f, (S)((S)cand - (S)(1 * e)));
    cand = __builtin_amdgcn_update_dpp((int)f, (int)f, 0x112, 0xf, 0xf, false);
    if ((lane & 15) >= 2) f = smax(f, (S)((S)cand - (S)(2 * e)));
    cand = __builtin_amdgcn_update_dpp((int)f, (int)f, 0x114, 0xf, 0xf, false);
    if ((lane & 15) >= 4) f = smax(f, (S)((S)cand - (S)(4 * e)));
    cand = __builtin_amdgcn_update_dpp((int)f, (int)f, 0x118, 0xf, 0xf, false);
    if ((lane & 15) >= 8) f = smax(f, (S)((S)cand - (S)(8 * e)));
    /* cross-row propagation: each row's full prefix ends at its last lane;
     * broadcast it (readlane, SALU) and decay by the per-lane distance.
     * r after each step covers all rows up to that boundary, so coverage is
     * complete (a plain +16/+32 jump after a row-local scan is NOT). */
    S r = (S)__builtin_amdgcn_readlane((int)f, 15);
    if (lane >= 16) f = smax(f, (S)(r - (S)((lane - 15) * e)));
    r = (S)__builtin_amdgcn_readlane((int)f, 31);
    if (lane >= 32) f = smax(f, (S)(r - (S)((lane - 31) * e)));
    r = (S)__builtin_amdgcn_readlane((int)f, 47);
    if (lane >= 48) f = smax(f, (S)(r - (S)((lane - 47) * e)));
    return f;
}

/* Wave-uniform max/min reductions: 4 DPP row_shr steps collect each 16-lane
 * row's reduction into its last lane, 4 readlanes + scalar ops finish — the
 * result is identical to a 6-step __shfl_xor tree but costs ~4 VALU + 4
 * SALU-ish ops instead of 18 DS-unit permutes (measured ~3.3k cycles per row
 * in the epilogue before this). bound_ctrl=false keeps the lane's own value
 * when the DPP source is out of range: the identity for max/min. */
__device__ __forceinline__ int wave_red_max_i32(int v) {
    int t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false); v = v > t ? v : t;
    int r0 = __builtin_amdgcn_readlane(v, 15), r1 = __builtin_amdgcn_readlane(v, 31);
    int r2 = __builtin_amdgcn_readlane(v, 47), r3 = __builtin_amdgcn_readlane(v, 63);
    r0 = r0 > r1 ? r0 : r1; r2 = r2 > r3 ? r2 : r3;
    return r0 > r2 ? r0 : r2;
}
__device__ __forceinline__ int wave_red_min_i32(int v) {
    int t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false); v = v < t ? v : t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false); v = v < t ? v : t;
    int r0 = __builtin_amdgcn_readlane(v, 15), r1 = __builtin_amdgcn_readlane(v, 31);
    int r2 = __builtin_amdgcn_readlane(v, 47), r3 = __builtin_amdgcn_readlane(v, 63);
    r0 = r0 < r1 ? r0 : r1; r2 = r2 < r3 ? r2 : r3;
    return r0 < r2 ? r0 : r2;
}

/* device push_cigar, matching abpoa_align.h:54-73 (run-length merge for I/S/H) */
__device__ static int dev_push_cigar(uint64_t *cig, int *n_c, int cap, int op, int len,
                                     int node_id, int query_id, int *status) {
    uint64_t l = (uint64_t)len;
    if (*n_c == 0 || (op != 1 /*I*/ && op != 4 && op != 5) || op != (int)(cig[*n_c - 1] & 0xf)) {
        if (*n_c >= cap) { *status = ABAMD_JOB_CIGAR_OVERFLOW; return -1; }
        uint64_t n_id = (uint64_t)(uint32_t)node_id, q_id = (uint64_t)(uint32_t)query_id;
        if (op == 0 || op == 3) cig[(*n_c)++] = n_id << 34 | q_id << 4 | (uint64_t)op;
        else if (op == 1 || op == 4 || op == 5) cig[(*n_c)++] = q_id << 34 | l << 4 | (uint64_t)op;
        else cig[(*n_c)++] = n_id << 34 | l << 4 | (uint64_t)op; /* D */
    } else cig[*n_c - 1] += l << 4;
    return 0;
}

/* ------------------------------------------------------------------ */
/* The multi-wave frame: ONE JOB PER 512-THREAD BLOCK, and what the     */
/* affine and linear kernels do around their recurrences, once. Every   */
/* thread of the block calls a helper with the same arguments unless    */
/* the helper says otherwise. No helper holds a barrier (the kernels    */
/* place them, and say what each one orders) and none knows which gap   */
/* model called it.                                                     */
/* ------------------------------------------------------------------ */

/* adaptive band state init (abpoa_topological_sort:347-353 + first_dp);
 * the caller's next barrier publishes it */
__device__ __forceinline__ void mw_steer_init(const abamd_gpu_job_t &jb, int tid) {
    for (int i = tid; i < jb.n_rows; i += MWT) {
        jb.max_left[i] = jb.node_n_init;
        jb.max_right[i] = 0;
    }
    if (tid == 0) { jb.max_left[0] = 0; jb.max_right[0] = 0; }
    for (int k = jb.out_off[0] + tid; k < jb.out_off[1]; k += MWT) {
        int o = jb.out_idx[k];
        jb.max_left[o] = 1; jb.max_right[o] = 1;
    }
}

/* band end of row 0 (GET_AD_DP_END, abpoa_align.h:35) */
__device__ __forceinline__ int mw_first_row_end(const abamd_gpu_job_t &jb, int end_remain) {
    if (!jb.banded) return jb.qlen;
    const int mr = jb.max_remain[0] - end_remain - 1;
    const int t = jb.max_right[0] > jb.qlen - mr ? jb.max_right[0] : jb.qlen - mr;
    return (jb.qlen < t + jb.w) ? jb.qlen : t + jb.w;
}

/* A row's scalars. The kernels load them one row ahead, so that the latency
 * hides under the previous row: `mw_row_t nxt` holds row r+1 while row r is
 * computed. A steering push r -> r+1 therefore never goes through memory:
 * max_left/max_right of row r+1 were loaded before row r could push, so the
 * push is merged into nxt (the same copy in every thread). */
struct mw_row_t {
    int pk0, pk1;       /* its predecessors: pre_idx[pk0 .. pk1) */
    int oo0, oo1;       /* its out-edges: out_idx[oo0 .. oo1) */
    int remain;         /* max_remain */
    int ml, mr;         /* max_left / max_right */
    int pidx0, ps0;     /* first predecessor and its path score */

    __device__ __forceinline__ void load(const abamd_gpu_job_t &jb, int r, int r_next) {
        pk1 = jb.pre_off[r_next];
        oo1 = jb.out_off[r_next];
        remain = jb.max_remain[r];
        ml = jb.max_left[r];
        mr = jb.max_right[r];
        pidx0 = jb.pre_idx[pk0];
        ps0 = jb.pre_ps[pk0];
    }
    __device__ __forceinline__ void first(const abamd_gpu_job_t &jb) { /* row 1 */
        pk0 = jb.pre_off[1];
        oo0 = jb.out_off[1];
        load(jb, 1, 2 <= jb.n_rows ? 2 : jb.n_rows);
    }
    __device__ __forceinline__ void advance(const abamd_gpu_job_t &jb, int r) { /* to row r */
        pk0 = pk1;
        oo0 = oo1;
        load(jb, r, r + 1);
    }
};

/* the row whose band the LDS previous-row cache holds, if any */
struct mw_prev_t { int ok, row, beg, end; };

/* adaptive band of a row (GET_AD_DP_BEGIN/END, abpoa_align.h:34-35): the
 * steering maxima of the row, widened by w, and never starting left of the
 * leftmost band start among its predecessors */
__device__ __forceinline__ void mw_row_band(const abamd_gpu_job_t &jb, const abamd_row_meta_t *meta,
                                            const mw_row_t &row, const mw_prev_t &prev,
                                            int end_remain, int &beg, int &end) {
    if (!jb.banded) { beg = 0; end = jb.qlen; return; }
    const int mr = row.remain - end_remain - 1;
    int lo = row.ml < jb.qlen - mr ? row.ml : jb.qlen - mr;
    beg = lo - jb.w; if (beg < 0) beg = 0;
    int hi = row.mr > jb.qlen - mr ? row.mr : jb.qlen - mr;
    end = hi + jb.w; if (end > jb.qlen) end = jb.qlen;
    int min_pre_beg;
    if (row.pk1 - row.pk0 == 1) {
        min_pre_beg = (prev.ok && row.pidx0 == prev.row) ? prev.beg : meta[row.pidx0].beg;
    } else {
        min_pre_beg = 0x7fffffff;
        for (int k = row.pk0; k < row.pk1; ++k) {
            const int pidx = jb.pre_idx[k];
            int pb = (prev.ok && pidx == prev.row) ? prev.beg : meta[pidx].beg;
            if (pb < min_pre_beg) min_pre_beg = pb;
        }
    }
    if (beg < min_pre_beg) beg = min_pre_beg;
}

/* Row argmax (simd_abpoa_max_in_row: leftmost and rightmost column of the
 * maximum). Each thread brings the maximum over its own cells; lane 0 of
 * every wave publishes the wave's into sc_red[3 * MWAVES]. The kernels call
 * this in a row's last superchunk, so the barrier that ends the superchunk
 * publishes it as well. */
struct mw_rowmax_t { int mv, ll, rr; };

/* the argmax steers the band and is the score of local and extension mode;
 * an unbanded global job needs none */
__device__ __forceinline__ bool mw_needs_rowmax(const abamd_gpu_job_t &jb) {
    return jb.banded || jb.align_mode == 1 || jb.align_mode == 2;
}

template <typename S>
__device__ __forceinline__ void mw_rowmax_publish(int *sc_red, int wv, int lane,
                                                  S lmax, int lleft, int lright) {
    int mvw = wave_red_max_i32((int)lmax);
    int llw = ((int)lmax == mvw && lleft >= 0) ? lleft : 0x7fffffff;
    int rrw = ((int)lmax == mvw && lright >= 0) ? lright : -1;
    llw = wave_red_min_i32(llw);
    rrw = wave_red_max_i32(rrw);
    if (lane == 0) {
        sc_red[wv] = mvw;
        sc_red[MWAVES + wv] = llw;
        sc_red[2 * MWAVES + wv] = rrw;
    }
}

/* every thread repeats the 8-way combine from LDS (uniform result) */
__device__ __forceinline__ mw_rowmax_t mw_rowmax_combine(const int *sc_red) {
    mw_rowmax_t m = { sc_red[0], sc_red[MWAVES], sc_red[2 * MWAVES] };
    #pragma unroll
    for (int ww = 1; ww < MWAVES; ++ww) {
        int m2 = sc_red[ww];
        if (m2 > m.mv) { m.mv = m2; m.ll = sc_red[MWAVES + ww]; m.rr = sc_red[2 * MWAVES + ww]; }
        else if (m2 == m.mv) {
            if (sc_red[MWAVES + ww] < m.ll) m.ll = sc_red[MWAVES + ww];
            if (sc_red[2 * MWAVES + ww] > m.rr) m.rr = sc_red[2 * MWAVES + ww];
        }
    }
    return m;
}

/* running best cell of local and extension mode (starts as { inf_min, 0, 0,
 * max_remain[0], 0 }); zdropped ends the row loop */
struct mw_best_t { int32_t score; int i, j, remain, zdropped; };

__device__ __forceinline__ void mw_best_update(const abamd_gpu_job_t &jb, mw_best_t &b,
                                               int r, int row_remain, const mw_rowmax_t &m) {
    if (jb.align_mode == 1) {
        if (m.mv > b.score) { b.score = m.mv; b.i = r; b.j = m.ll; }
    } else if (jb.align_mode == 2) {
        if (m.mv > b.score) {
            b.score = m.mv; b.i = r; b.j = m.rr;
            b.remain = row_remain;
        } else if (jb.zdrop > 0) {
            int delta = b.remain - row_remain;
            int dd = delta - (m.rr - b.j); if (dd < 0) dd = -dd;
            if (b.score - m.mv > jb.zdrop + jb.e1 * dd) b.zdropped = 1;
        }
    }
}

/* band steering: row r pushes its argmax columns to its out-edges; nxt
 * holds row r+1. Every thread performs the same idempotent update, so its
 * own later load of max_left/max_right of row o is self-ordered. */
__device__ __forceinline__ void mw_steer_push(const abamd_gpu_job_t &jb, const mw_row_t &row, int r,
                                              const mw_rowmax_t &m, mw_row_t &nxt) {
    for (int k = row.oo0; k < row.oo1; ++k) {
        int o = jb.out_idx[k];
        if (o == r + 1) {
            if (m.rr + 1 > nxt.mr) nxt.mr = m.rr + 1;
            if (m.ll + 1 < nxt.ml) nxt.ml = m.ll + 1;
        } else {
            if (m.rr + 1 > jb.max_right[o]) jb.max_right[o] = m.rr + 1;
            if (m.ll + 1 < jb.max_left[o]) jb.max_left[o] = m.ll + 1;
        }
    }
}

/* What follows the last barrier of row r: combine the published argmax, keep
 * the running best, push the steering to the out-edges. Returns nonzero
 * when the z-drop ends the row loop. */
__device__ __forceinline__ int mw_row_close(const abamd_gpu_job_t &jb, const int *sc_red,
                                            const mw_row_t &row, int r, mw_best_t &run,
                                            mw_row_t &nxt) {
    if (!mw_needs_rowmax(jb)) return 0;
    const mw_rowmax_t rm = mw_rowmax_combine(sc_red);
    mw_best_update(jb, run, r, row.remain, rm);
    if (run.zdropped) return 1;
    if (jb.banded) mw_steer_push(jb, row, r, rm, nxt);
    return 0;
}

/* Reserve row r's band [beg, end] in the arena (`used` counts cells per
 * plane) and record it in row_meta. Returns the row's offset, or -1 when the
 * arena is full. */
__device__ __forceinline__ int64_t mw_row_reserve(const abamd_gpu_job_t &jb, abamd_row_meta_t *meta,
                                                  int tid, int r, int beg, int end, int64_t &used) {
    const int64_t bw = end - beg + 1;
    if (used + bw > jb.arena_cap) return -1;
    const int64_t off = used;
    if (tid == 0) { meta[r].beg = beg; meta[r].end = end; meta[r].off = off; }
    used += bw;
    return off;
}

/* Where the backtrack starts: the running best, or in global mode the best
 * H at the band end of the sink's predecessors. `planes` is the number of
 * planes a row takes in the arena. */
template <typename S>
__device__ __forceinline__ void mw_final_best(const abamd_gpu_job_t &jb, const mw_best_t &run, int planes,
                                              int32_t &best_score, int &best_i, int &best_j) {
    best_score = run.score; best_i = run.i; best_j = run.j;
    if (jb.align_mode != 0) return;
    const abamd_row_meta_t *meta = (const abamd_row_meta_t*)jb.row_meta;
    best_score = jb.inf_min; best_i = 0; best_j = 0;
    for (int k = jb.pre_off[jb.n_rows - 1]; k < jb.pre_off[jb.n_rows]; ++k) {
        const int p = jb.pre_idx[k];
        const abamd_row_meta_t pm = meta[p];
        int e = pm.end < jb.qlen ? pm.end : jb.qlen;
        const S *pH = (const S*)jb.arena + pm.off * planes;
        int32_t sc = (e >= pm.beg) ? (int32_t)pH[e - pm.beg] : jb.inf_min;
        if (sc > best_score) { best_score = sc; best_i = p; best_j = e; }
    }
}

/* The backtrack walk of one thread, from cell (best_i, best_j) towards the
 * source: position, CIGAR under construction and the counters the result
 * reports. */
struct mw_walk_t {
    int bi, bj, id;         /* row, column, node id of the row */
    int start_i, start_j;   /* last cell visited */
    int look_end, put_right;
    int n_c, status, n_aln, n_matched;
};

__device__ __forceinline__ mw_walk_t mw_walk_begin(const abamd_gpu_job_t &jb, int best_i, int best_j) {
    mw_walk_t wk = { best_i, best_j, jb.row_node_id[best_i], best_i, best_j,
                     jb.put_gap_at_end, jb.put_gap_on_right, 0, ABAMD_JOB_OK, 0, 0 };
    if (best_j < jb.qlen)
        dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 1, jb.qlen - best_j, -1, jb.qlen - 1, &wk.status);
    return wk;
}

/* match step: the first predecessor p (of pre_idx[pq0 .. pq1), the row's)
 * with H[p][bj-1] + s + path score == Hj takes the walk to (p, bj-1).
 * Returns whether there was one. */
template <typename S>
__device__ __forceinline__ int mw_walk_match(const abamd_gpu_job_t &jb, mw_walk_t &wk, int planes,
                                             int pq0, int pq1, S s, int is_match, S Hj) {
    const abamd_row_meta_t *meta = (const abamd_row_meta_t*)jb.row_meta;
    for (int k = pq0; k < pq1; ++k) {
        const int p = jb.pre_idx[k];
        const S ps = (S)jb.pre_ps[k];
        const abamd_row_meta_t pm = meta[p];
        if (wk.bj - 1 < pm.beg || wk.bj - 1 > pm.end) continue;
        const S *pH = (const S*)jb.arena + pm.off * planes;
        if ((S)(pH[wk.bj - 1 - pm.beg] + s + ps) == Hj) {
            dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 0, 1, wk.id, wk.bj - 1, &wk.status);
            wk.bi = p; --wk.bj; wk.id = jb.row_node_id[wk.bi];
            ++wk.n_aln; wk.n_matched += is_match;
            return 1;
        }
    }
    return 0;
}

/* close the CIGAR (leading insertion when the walk stopped at column bj > 0)
 * and write the job's result */
__device__ __forceinline__ void mw_walk_end(const abamd_gpu_job_t &jb, abamd_gpu_res_t *res,
                                            mw_walk_t &wk, int best_i, int best_j) {
    if (wk.status == ABAMD_JOB_OK && wk.bj > 0)
        dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 1, wk.bj, -1, wk.bj - 1, &wk.status);
    res->status = wk.status;
    res->n_cigar = wk.n_c;
    res->n_aln_bases = wk.n_aln;
    res->n_matched_bases = wk.n_matched;
    res->node_e = jb.row_node_id[best_i]; res->query_e = best_j - 1;
    res->node_s = jb.row_node_id[wk.start_i]; res->query_s = wk.start_j - 1;
}

/* ------------------------------------------------------------------ */
/* Multi-wave convex kernel: ONE JOB PER 512-THREAD BLOCK.              */
/*                                                                      */
/* Round 1 ran one wavefront per job and was instruction-ISSUE bound: a */
/* lone wave on a SIMD issues one VALU op per 4 cycles, and a ~350-     */
/* instruction chunk body made a typical 340-cell row cost ~21k cycles. */
/* Here 8 waves cover the whole band at once: the M/E gather, H fold,   */
/* stores and argmax are embarrassingly lane-parallel, and the F        */
/* (insertion) max-plus chain splits into per-wave local scans plus a   */
/* cross-wave carry recurrence over the 8 published wave edges — the    */
/* regrouped decays are bit-identical because wrapping addition is      */
/* associative and the inf_min headroom (+512*ext_max, the same margin  */
/* the reference's vector code relies on) keeps every comparison        */
/* un-wrapped.                                                          */
/* Three block barriers per row replace ~5 serial chunk iterations.     */
/*                                                                      */
/* Row ring. Only the first few reads see a chain-like graph: after     */
/* read 10 of a 50 x 10 kbp set 60 % of the rows have a predecessor     */
/* that is not row r-1, after read 50 it is 91 % (the Kahn BFS          */
/* interleaves the variant branches), but 99 % of those references      */
/* reach back at most 10 rows. So the H/E1/E2 bands of the last         */
/* MW_RING rows stay in LDS, slot = row % MW_RING, with a               */
/* {row, beg, end} entry per slot (row = -1 when the band was wider     */
/* than a slot). A predecessor p with r - p <= dp_ring and a valid slot */
/* is gathered from LDS and gives its band start from the slot table;   */
/* anything else reads row_meta and the arena. Every value in the ring  */
/* is the value the arena holds, so the switch (job field dp_ring, 1 =  */
/* previous row only) does not change a single cell.                    */
/* Ordering: row r writes only slot r % MW_RING, data and table entry,  */
/* after its barrier B2. That slot held row r - MW_RING; the oldest row */
/* anyone still reads is r - MW_RING + 1 (by row r itself, before B1),  */
/* and rows < r finished their gathers before their own B1. B3 orders   */
/* the writes before row r+1's reads. The first three predecessors of a */
/* row are rolled one row ahead like the other row scalars; their ring  */
/* or row_meta lookups are done once per row and shared by the band     */
/* start (min_pre_beg) and the gather.                                  */
/* ------------------------------------------------------------------ */
/* ring slots: rows r-1 .. r-ABAMD_DP_RING_MAX are readable while row r is
 * written. int32: 11 x 3 x 512 x 4 B = 66 KiB (+3 KiB matrix), under the
 * 80 KiB that keeps two blocks per CU; int16 takes half. Depth 10 is where
 * one more slot adds less than one point of coverage after read 50
 * (d<=8 96.9 %, d<=10 99.1 %, d<=12 99.75 % of the far references). */
#define MW_RING (ABAMD_DP_RING_MAX + 1)
/* predecessors (and out-edges) per row rolled one row ahead: 3 keeps the
 * int32 instantiation at 104 VGPRs, which leaves a fold wave (72) room on a
 * SIMD next to four DP waves; 4 costs 106 (112 allocated) */
#define MW_NPF 3

/* one predecessor row as the gather sees it: slot >= 0 -> LDS ring */
struct mw_pred_t { int slot, beg, end; };

/* FAST is the north-star instantiation: global mode, banded, no path scores,
 * ring at full depth. Those job fields are then compile-time constants, so
 * the row loop carries none of the tests or of the state (running best,
 * z-drop flag, ring depth, path-score switch) that serve the other modes.
 * The host picks the instantiation per launch from the fields it writes into
 * the jobs (abamd_cg_fast_eligible); FAST = false is the kernel for
 * everything else. */
template <typename S, bool FAST>
__global__ __launch_bounds__(MWT, 4) /* 4 waves/SIMD: two blocks per CU */
void cg_global_mw_kernel(const abamd_gpu_job_t *__restrict__ jobs,
                         abamd_gpu_res_t *__restrict__ results, int n_jobs) {
    const int jid = blockIdx.x;
    if (jid >= n_jobs) return;
    const int tid = threadIdx.x;
    const int wv = tid / WAVE, lane = tid % WAVE;

    __shared__ int mat_lds[27 * 27];
    __shared__ S ring_lds[MW_RING][3 * BMW];
    __shared__ int4 ring_tbl[MW_RING]; /* {row or -1, beg, end, 0} per slot */
    __shared__ S sc_h[MWAVES], sc_f1[MWAVES], sc_f2[MWAVES];
    __shared__ int sc_red[3 * MWAVES];
    __shared__ S sc_carry[3];

    const abamd_gpu_job_t jb = jobs[jid];
    abamd_gpu_res_t *res = &results[jid];
    abamd_row_meta_t *__restrict__ meta = (abamd_row_meta_t*)jb.row_meta;

    const int qlen = jb.qlen, n_rows = jb.n_rows, w = jb.w, m = jb.m;
    const S inf_min = (S)jb.inf_min;
    const S e1 = (S)jb.e1, e2 = (S)jb.e2;
    const S oe1 = (S)jb.oe1, oe2 = (S)jb.oe2;
    const bool local_mode = !FAST && jb.align_mode == 1;
    const bool extend_mode = !FAST && jb.align_mode == 2;
    const bool banded = FAST || jb.banded;
    int32_t run_best = jb.inf_min;
    int run_best_i = 0, run_best_j = 0, run_best_remain = jb.max_remain[0];
    int zdropped = 0;
    const int end_remain = jb.max_remain[n_rows - 1];
    S *arena = (S*)jb.arena;
    const uint8_t *__restrict__ query = jb.query;
    /* The job's arrays again as global-address-space pointers for the row
     * loop. Pointers loaded from the job struct are generic, and generic
     * (flat) loads and stores count on the LDS counter as well: every LDS
     * wait of a row, the first ring read included, then also waited for the
     * rolled global loads issued just above it and for the previous row's
     * plane stores. */
    typedef __attribute__((address_space(1))) S GS;
    typedef __attribute__((address_space(1))) int gint_t;
    typedef __attribute__((address_space(1))) uint8_t gu8_t;
    typedef __attribute__((address_space(1))) abamd_row_meta_t gmeta_t;
    /* FAST reads the row CSR and max_remain through constant-address-space
     * pointers: an earlier kernel or copy wrote them and this kernel only
     * reads them, so the scalar cache is coherent, and a load at a uniform
     * index (every rolled one is) becomes a scalar load straight into SGPRs
     * with scalar address arithmetic: no VALU address chain, no VGPR and no
     * lane read per value. max_left, max_right and row_meta are written here
     * and stay vector accesses. */
    typedef __attribute__((address_space(4))) int cint_t;
    typedef typename std::conditional<FAST, cint_t, gint_t>::type rint_t;
    GS *const g_arena = (GS*)jb.arena;
    const gu8_t *const g_query = (const gu8_t*)jb.query;
    const gu8_t *const g_row_base = (const gu8_t*)jb.row_base;
    const rint_t *const g_pre_off = (const rint_t*)jb.pre_off;
    const rint_t *const g_pre_idx = (const rint_t*)jb.pre_idx;
    const gint_t *const g_pre_ps = (const gint_t*)jb.pre_ps;
    const rint_t *const g_out_off = (const rint_t*)jb.out_off;
    const rint_t *const g_out_idx = (const rint_t*)jb.out_idx;
    const rint_t *const g_max_remain = (const rint_t*)jb.max_remain;
    gint_t *const g_max_left = (gint_t*)jb.max_left;
    gint_t *const g_max_right = (gint_t*)jb.max_right;
    gmeta_t *const g_meta = (gmeta_t*)jb.row_meta;

    for (int i = tid; i < m * m; i += MWT) mat_lds[i] = jb.mat[i];
    if (tid == 0) { res->status = ABAMD_JOB_OK; res->n_cigar = 0; }

    /* adaptive band state init (abpoa_topological_sort:347-353 + first_dp) */
    for (int i = tid; i < n_rows; i += MWT) {
        g_max_left[i] = jb.node_n_init;
        g_max_right[i] = 0;
    }
    if (tid == 0) { g_max_left[0] = 0; g_max_right[0] = 0; }
    for (int k = g_out_off[0] + tid; k < g_out_off[1]; k += MWT) {
        int o = g_out_idx[k];
        g_max_left[o] = 1; g_max_right[o] = 1;
    }
    if (tid < MW_RING) ring_tbl[tid] = make_int4(-1, 0, -1, 0);
    __syncthreads();

    const int depth = FAST ? ABAMD_DP_RING_MAX
                    : jb.dp_ring < 1 ? 1
                    : (jb.dp_ring > ABAMD_DP_RING_MAX ? ABAMD_DP_RING_MAX : jb.dp_ring);
    const int ips = FAST ? 0 : jb.inc_path_score;
    const int pre_last = g_pre_off[n_rows] - 1; /* clamps for the rolled loads */
    const int out_last = g_out_off[n_rows] - 1;

    /* ---- first row (simd_abpoa_cg_first_dp) ---- */
    int64_t used;
    {
        int mr = g_max_remain[0] - end_remain - 1;
        int end0;
        if (banded) {
            int t = g_max_right[0] > qlen - mr ? g_max_right[0] : qlen - mr;
            end0 = (qlen < t + w) ? qlen : t + w;
        } else end0 = qlen;
        if (tid == 0) { g_meta[0].beg = 0; g_meta[0].end = end0; g_meta[0].off = 0; }
        int64_t bw = end0 + 1;
        used = bw;
        /* 3 planes only (H,E1,E2): the F planes are recomputed from stored H
         * at backtrack time (validated: tools/f_recompute_experiment.py — a
         * 40% cut of plane bytes and arena capacity) */
        GS *H = g_arena, *E1 = g_arena + bw, *E2 = g_arena + 2 * bw;
        S *c = &ring_lds[0][0];
        const int fits = end0 + 1 <= BMW;
        for (int j = tid; j <= end0; j += MWT) {
            S hv, e1v2, e2v2;
            if (local_mode) {
                hv = 0; e1v2 = 0; e2v2 = 0;
            } else if (j == 0) {
                hv = 0; e1v2 = (S)(0 - oe1); e2v2 = (S)(0 - oe2);
            } else {
                S f1 = (S)(-(jb.o1 + jb.e1 * j));
                S f2 = (S)(-(jb.o2 + jb.e2 * j));
                hv = smax(f1, f2);
                e1v2 = inf_min; e2v2 = inf_min;
            }
            H[j] = hv; E1[j] = e1v2; E2[j] = e2v2;
            if (fits) {
                c[j] = hv; c[BMW + j] = e1v2; c[2 * BMW + j] = e2v2;
            }
        }
        if (tid == 0) ring_tbl[0] = make_int4(fits ? 0 : -1, 0, end0, 0);
        __syncthreads();
    }

    /* ---- main row loop (row scalars rolled one row ahead; the common
     * band push r -> r+1 carried in registers — every thread keeps the
     * same copy, and skip-edge pushes are idempotent same-value writes
     * done by every thread so each thread's later prefetch of the pushed
     * row is self-ordered) ---- */
    int cur_pk0 = g_pre_off[1];
    int cur_pk1 = g_pre_off[2 <= n_rows ? 2 : n_rows];
    int cur_oo0 = g_out_off[1];
    int cur_oo1 = g_out_off[2 <= n_rows ? 2 : n_rows];
    int cur_remain = g_max_remain[1];
    int cur_ml_mem = g_max_left[1];
    int cur_mr_mem = g_max_right[1];
    /* the first MW_NPF predecessor indices, loaded unconditionally (index
     * clamped into the array) so they do not wait for the row's pre_off */
    int cur_pidx[MW_NPF];
    #pragma unroll
    for (int i = 0; i < MW_NPF; ++i) {
        int k = cur_pk0 + i; if (k > pre_last) k = pre_last; if (k < 0) k = 0;
        cur_pidx[i] = g_pre_idx[k];
    }
    int cur_oidx[MW_NPF];
    #pragma unroll
    for (int i = 0; i < MW_NPF; ++i) {
        int k = cur_oo0 + i; if (k > out_last) k = out_last; if (k < 0) k = 0;
        cur_oidx[i] = g_out_idx[k];
    }
    int cur_base = g_row_base[1];
    int push_ml = 0x7fffffff, push_mr = -0x7fffffff;
    int slot = 0; /* r % MW_RING */
#ifdef ABAMD_KPROF
    unsigned long long mw_a = 0, mw_b = 0, mw_c = 0, mw_d = 0, mw_rows = 0;
#endif
    for (int r = 1; r < n_rows - 1; ++r) {
        KPROF_T(mt0);
        if (++slot == MW_RING) slot = 0;
        const int pk0 = cur_pk0, pk1 = cur_pk1;
        const int oo0 = cur_oo0, oo1 = cur_oo1;
        const int row_remain = cur_remain;
        int pidx[MW_NPF], oidx[MW_NPF];
        #pragma unroll
        for (int i = 0; i < MW_NPF; ++i) {
            pidx[i] = __builtin_amdgcn_readfirstlane(cur_pidx[i]);
            oidx[i] = __builtin_amdgcn_readfirstlane(cur_oidx[i]);
        }
        const int base = cur_base;
        const int ml_eff = cur_ml_mem < push_ml ? cur_ml_mem : push_ml;
        const int mr_eff = cur_mr_mem > push_mr ? cur_mr_mem : push_mr;
        {
            const int nr = r + 1;
            cur_pk0 = pk1;
            cur_pk1 = g_pre_off[nr + 1];
            cur_oo0 = oo1;
            cur_oo1 = g_out_off[nr + 1];
            cur_remain = g_max_remain[nr];
            cur_ml_mem = g_max_left[nr];
            cur_mr_mem = g_max_right[nr];
            cur_base = g_row_base[nr];
            #pragma unroll
            for (int i = 0; i < MW_NPF; ++i) {
                int k = cur_pk0 + i; if (k > pre_last) k = pre_last; if (k < 0) k = 0;
                cur_pidx[i] = g_pre_idx[k];
                k = cur_oo0 + i; if (k > out_last) k = out_last; if (k < 0) k = 0;
                cur_oidx[i] = g_out_idx[k];
            }
            /* FAST: all nine scalar loads in flight before the first wait:
             * without this every result is moved to its spill lane at once,
             * each behind a wait of its own */
            if (FAST)
                asm volatile("" :: "s"(cur_pk1), "s"(cur_oo1), "s"(cur_remain),
                             "s"(cur_pidx[0]), "s"(cur_pidx[1]), "s"(cur_pidx[2]),
                             "s"(cur_oidx[0]), "s"(cur_oidx[1]), "s"(cur_oidx[2]));
        }
        /* predecessor lookup: ring slot table first (one LDS read), else
         * row_meta. Uniform across the block; readfirstlane keeps the
         * results in scalar registers. */
        const int npre = pk1 - pk0;
        auto ring_probe = [&](int p, int4 &t) -> int { /* slot index to test */
            const int d = r - p;
            int s = slot - ((d >= 1 && d <= ABAMD_DP_RING_MAX) ? d : 0);
            if (s < 0) s += MW_RING;
            t = ring_tbl[s];
            return s;
        };
        auto pred_resolve = [&](int p, int s, const int4 &t, mw_pred_t &q) {
            const int d = r - p;
            if (d >= 1 && d <= depth && __builtin_amdgcn_readfirstlane(t.x) == p) {
                q.slot = s;
                q.beg = __builtin_amdgcn_readfirstlane(t.y);
                q.end = __builtin_amdgcn_readfirstlane(t.z);
            } else { /* rare: the gather re-reads row_meta for end and offset */
                q.slot = -1;
                q.beg = __builtin_amdgcn_readfirstlane(g_meta[p].beg);
                q.end = -1;
            }
        };
        mw_pred_t pf[MW_NPF];
        int min_pre_beg = 0x7fffffff;
        {
            int4 pt[MW_NPF]; int psl[MW_NPF];
            #pragma unroll
            for (int i = 0; i < MW_NPF; ++i) psl[i] = ring_probe(pidx[i], pt[i]);
            #pragma unroll
            for (int i = 0; i < MW_NPF; ++i) {
                pf[i].slot = -1; pf[i].beg = 0; pf[i].end = -1;
                if (i < npre) {
                    pred_resolve(pidx[i], psl[i], pt[i], pf[i]);
                    if (pf[i].beg < min_pre_beg) min_pre_beg = pf[i].beg;
                }
            }
            for (int k = pk0 + MW_NPF; k < pk1; ++k) {
                const int p = g_pre_idx[k];
                int4 t; mw_pred_t q;
                const int s = ring_probe(p, t);
                pred_resolve(p, s, t, q);
                if (q.beg < min_pre_beg) min_pre_beg = q.beg;
            }
        }
#ifdef ABAMD_KPROF
        /* row class by what a full-depth ring would serve, whatever dp_ring
         * is: 0 = single predecessor r-1 in the ring, 1 = every predecessor
         * in the ring, 2 = at least one arena gather */
        int kp_cls;
        unsigned long long kp_a = 0;
        {
            int n_far = 0;
            for (int k = pk0; k < pk1; ++k) {
                const int p = g_pre_idx[k];
                int4 t; (void)ring_probe(p, t);
                const int d = r - p;
                if (!(d >= 1 && d <= ABAMD_DP_RING_MAX && t.x == p)) ++n_far;
            }
            kp_cls = n_far ? 2 : ((npre == 1 && pidx[0] == r - 1) ? 0 : 1);
        }
#endif
        int beg, end;
        {
            int mr = row_remain - end_remain - 1;
            if (banded) {
                int lo = ml_eff < qlen - mr ? ml_eff : qlen - mr;
                beg = lo - w; if (beg < 0) beg = 0;
                int hi = mr_eff > qlen - mr ? mr_eff : qlen - mr;
                end = hi + w; if (end > qlen) end = qlen;
                if (beg < min_pre_beg) beg = min_pre_beg;
            } else { beg = 0; end = qlen; }
        }
        const int64_t bw = end - beg + 1;
        if (used + bw > jb.arena_cap) { if (tid == 0) res->status = ABAMD_JOB_ARENA_OVERFLOW; return; }
        const int64_t off = used;
        if (tid == 0) { g_meta[r].beg = beg; g_meta[r].end = end; g_meta[r].off = off; }
        used += bw;
        GS *H = g_arena + off * 3, *E1r = H + bw, *E2r = E1r + bw;
        const int *mrow = &mat_lds[base * m];
        const int cache_fits = bw <= BMW;
        S *cw = &ring_lds[slot][0];

        S carry_h = inf_min, f1c = inf_min, f2c = inf_min; /* superchunk carries */
        S lmax = inf_min; int lleft = -1, lright = -1;

        for (int ss = beg; ss <= end; ss += MWT) {
            const int j = ss + tid;
            const bool act = j <= end;
            S h = inf_min, e1v = inf_min, e2v = inf_min;
            auto gather = [&](const int p, const mw_pred_t &q, const S ps) {
                if (q.slot >= 0) {
                    const S *cr = &ring_lds[q.slot][0];
                    if (act) {
                        if (local_mode && j == 0) { if (ps > h) h = ps; }
                        if (j - 1 >= q.beg && j - 1 <= q.end) {
                            S v = (S)(cr[j - 1 - q.beg] + ps);
                            if (v > h) h = v;
                        }
                        if (j >= q.beg && j <= q.end) {
                            S v1 = (S)(cr[BMW + j - q.beg] + ps);
                            S v2 = (S)(cr[2 * BMW + j - q.beg] + ps);
                            if (v1 > e1v) e1v = v1;
                            if (v2 > e2v) e2v = v2;
                        }
                    }
                    return;
                }
                abamd_row_meta_t pm;
                pm.beg = g_meta[p].beg; pm.end = g_meta[p].end; pm.off = g_meta[p].off;
                const int64_t pbw = pm.end - pm.beg + 1;
                const GS *__restrict__ pH = g_arena + pm.off * 3;
                const GS *__restrict__ pE1 = pH + pbw;
                const GS *__restrict__ pE2 = pE1 + pbw;
                if (act) {
                    if (local_mode && j == 0) { if (ps > h) h = ps; }
                    if (j - 1 >= pm.beg && j - 1 <= pm.end) {
                        S v = (S)(pH[j - 1 - pm.beg] + ps);
                        if (v > h) h = v;
                    }
                    if (j >= pm.beg && j <= pm.end) {
                        S v1 = (S)(pE1[j - pm.beg] + ps);
                        S v2 = (S)(pE2[j - pm.beg] + ps);
                        if (v1 > e1v) e1v = v1;
                        if (v2 > e2v) e2v = v2;
                    }
                }
            };
            /* pre_ps is all zero unless inc_path_score: skip its loads */
            #pragma unroll
            for (int i = 0; i < MW_NPF; ++i)
                if (i < npre) gather(pidx[i], pf[i], ips ? (S)g_pre_ps[pk0 + i] : (S)0);
            for (int k = pk0 + MW_NPF; k < pk1; ++k) {
                const int p = g_pre_idx[k];
                int4 t; mw_pred_t q;
                const int s = ring_probe(p, t);
                pred_resolve(p, s, t, q);
                gather(p, q, ips ? (S)g_pre_ps[k] : (S)0);
            }
            const S q = (S)((j == 0 || !act) ? 0 : mrow[g_query[j - 1]]);
            S hpre = (S)(h + q);
            hpre = smax(hpre, smax(e1v, e2v));
            if (!act) hpre = inf_min;

            /* wave edges of hpre, then per-wave local F scans */
            KPROF_T(mt1);
            if (lane == WAVE - 1) sc_h[wv] = hpre;
            __syncthreads();
            S hshift = (S)__shfl_up((int)hpre, 1);
            S c1, c2;
            if (lane == 0) {
                if (wv == 0) {
                    if (ss == beg) { c1 = (S)(inf_min - oe1); c2 = (S)(inf_min - oe2); }
                    else {
                        c1 = smax((S)(carry_h - oe1), (S)(f1c - e1));
                        c2 = smax((S)(carry_h - oe2), (S)(f2c - e2));
                    }
                } else {
                    S hp = sc_h[wv - 1];
                    c1 = (S)(hp - oe1);
                    c2 = (S)(hp - oe2);
                }
            } else {
                c1 = (S)(hshift - oe1);
                c2 = (S)(hshift - oe2);
            }
            S L1 = scan_maxplus(c1, jb.e1, inf_min, lane);
            S L2 = scan_maxplus(c2, jb.e2, inf_min, lane);
            if (lane == WAVE - 1) { sc_f1[wv] = L1; sc_f2[wv] = L2; }
            __syncthreads();
            /* cross-wave carry: C = true F at the last lane of wave wv-1
             * (max-plus with linear decay is associative; wrapping adds
             * regroup exactly) */
            S f1 = L1, f2 = L2;
            if (wv > 0) {
                S C1 = sc_f1[0], C2 = sc_f2[0];
                for (int ww = 1; ww < wv; ++ww) {
                    C1 = smax(sc_f1[ww], (S)(C1 - (S)(WAVE * jb.e1)));
                    C2 = smax(sc_f2[ww], (S)(C2 - (S)(WAVE * jb.e2)));
                }
                f1 = smax(L1, (S)(C1 - (S)((lane + 1) * jb.e1)));
                f2 = smax(L2, (S)(C2 - (S)((lane + 1) * jb.e2)));
            }

            S hf = smax(hpre, smax(f1, f2));
            if (local_mode) hf = smax(hf, (S)0);
            S e1n = smax((S)(e1v - e1), (S)(hf - oe1));
            S e2n = smax((S)(e2v - e2), (S)(hf - oe2));
            if (local_mode) { e1n = smax(e1n, (S)0); e2n = smax(e2n, (S)0); }
            if (act) {
                H[j - beg] = hf; E1r[j - beg] = e1n; E2r[j - beg] = e2n;
                if (cache_fits) {
                    cw[j - beg] = hf;
                    cw[BMW + j - beg] = e1n;
                    cw[2 * BMW + j - beg] = e2n;
                }
                if (hf > lmax) { lmax = hf; lleft = j; lright = j; }
                else if (hf == lmax) { lright = j; }
            }
            KPROF_T(mt2);
            const bool more = ss + MWT <= end;
            if (more && j == ss + MWT - 1) {
                sc_carry[0] = hpre; sc_carry[1] = f1; sc_carry[2] = f2;
            }
            /* this row's slot entry: after B2, so every gather of this row
             * (none of which reads this slot) has passed; B3 publishes it */
            if (!more && tid == 0)
                ring_tbl[slot] = make_int4(cache_fits ? r : -1, beg, end, 0);
            if (!more && (banded || local_mode || extend_mode)) {
                /* last superchunk: fold the per-wave argmax publish into this
                 * barrier instead of paying a fourth barrier (and its store
                 * drain) after the loop */
                int mvw = wave_red_max_i32((int)lmax);
                int llw = ((int)lmax == mvw && lleft >= 0) ? lleft : 0x7fffffff;
                int rrw = ((int)lmax == mvw && lright >= 0) ? lright : -1;
                llw = wave_red_min_i32(llw);
                rrw = wave_red_max_i32(rrw);
                if (lane == 0) {
                    sc_red[wv] = mvw;
                    sc_red[MWAVES + wv] = llw;
                    sc_red[2 * MWAVES + wv] = rrw;
                }
            }
            __syncthreads(); /* also orders cw writes before the next row's reads */
            if (more) { carry_h = sc_carry[0]; f1c = sc_carry[1]; f2c = sc_carry[2]; }
#ifdef ABAMD_KPROF
            {
                unsigned long long mt3 = __builtin_readcyclecounter();
                mw_a += mt1 - mt0;   /* band + prefetch + gather + hpre */
                mw_b += mt2 - mt1;   /* B1 + scans + B2 + carries + fold + stores */
                mw_c += mt3 - mt2;   /* carry publish + B3 */
                kp_a += mt1 - mt0;
            }
#endif
        }
        KPROF_T(mt3e);

        if (banded || local_mode || extend_mode) {
            /* per-wave argmax published under the loop's last barrier; every
             * thread repeats the 8-way combine from LDS (uniform result) */
            int mv = sc_red[0], ll = sc_red[MWAVES], rr = sc_red[2 * MWAVES];
            #pragma unroll
            for (int ww = 1; ww < MWAVES; ++ww) {
                int m2 = sc_red[ww];
                if (m2 > mv) { mv = m2; ll = sc_red[MWAVES + ww]; rr = sc_red[2 * MWAVES + ww]; }
                else if (m2 == mv) {
                    if (sc_red[MWAVES + ww] < ll) ll = sc_red[MWAVES + ww];
                    if (sc_red[2 * MWAVES + ww] > rr) rr = sc_red[2 * MWAVES + ww];
                }
            }
            if (local_mode) {
                if (mv > run_best) { run_best = mv; run_best_i = r; run_best_j = ll; }
            } else if (extend_mode) {
                if (mv > run_best) {
                    run_best = mv; run_best_i = r; run_best_j = rr;
                    run_best_remain = row_remain;
                } else if (jb.zdrop > 0) {
                    int delta = run_best_remain - row_remain;
                    int dd = delta - (rr - run_best_j); if (dd < 0) dd = -dd;
                    if (run_best - mv > jb.zdrop + jb.e1 * dd) zdropped = 1;
                }
            }
            push_ml = 0x7fffffff; push_mr = -0x7fffffff;
            if (!zdropped && banded) {
                /* every thread performs the same idempotent update so its
                 * own later prefetch of row o is self-ordered */
                auto push = [&](const int o) {
                    if (o == r + 1) {
                        if (rr + 1 > push_mr) push_mr = rr + 1;
                        if (ll + 1 < push_ml) push_ml = ll + 1;
                    } else {
                        if (rr + 1 > g_max_right[o]) g_max_right[o] = rr + 1;
                        if (ll + 1 < g_max_left[o]) g_max_left[o] = ll + 1;
                    }
                };
                #pragma unroll
                for (int i = 0; i < MW_NPF; ++i)
                    if (i < oo1 - oo0) push(oidx[i]);
                for (int k = oo0 + MW_NPF; k < oo1; ++k) push(g_out_idx[k]);
            }
            if (zdropped) break;
        } else {
            push_ml = 0x7fffffff; push_mr = -0x7fffffff;
        }
#ifdef ABAMD_KPROF
        {
            unsigned long long mt4 = __builtin_readcyclecounter();
            mw_d += mt4 - mt0; mw_rows += 1; /* mt0 re-read below start */
            if (tid == 0) {
                atomicAdd(&abamd_kprof_acc[16 + kp_cls], 1ull);
                atomicAdd(&abamd_kprof_acc[19 + kp_cls], kp_a);
                atomicAdd(&abamd_kprof_acc[22 + kp_cls], mt4 - mt3e);
                atomicAdd(&abamd_kprof_acc[25 + kp_cls], mt4 - mt0);
                if (!cache_fits) atomicAdd(&abamd_kprof_acc[28], 1ull);
                if (npre > MW_NPF) atomicAdd(&abamd_kprof_acc[29], 1ull);
                atomicAdd(&abamd_kprof_acc[30], (unsigned long long)npre);
            }
        }
#endif
    }
#ifdef ABAMD_KPROF
    if (tid == 0) {
        atomicAdd(&abamd_kprof_acc[11], mw_a);
        atomicAdd(&abamd_kprof_acc[12], mw_b);
        atomicAdd(&abamd_kprof_acc[13], mw_c);
        atomicAdd(&abamd_kprof_acc[14], mw_d);
        atomicAdd(&abamd_kprof_acc[15], mw_rows);
    }
#endif

    __syncthreads();
    if (tid == 0) res->cells = used;

    /* ---- final best (computed redundantly by every thread: all inputs are
     * uniform, and every thread must stay alive for the cooperative
     * F-recompute below) ---- */
    int32_t best_score = run_best;
    int best_i = run_best_i, best_j = run_best_j;
    if (FAST || jb.align_mode == 0) {
        best_score = jb.inf_min; best_i = 0; best_j = 0;
        for (int k = jb.pre_off[n_rows - 1]; k < jb.pre_off[n_rows]; ++k) {
            const int p = jb.pre_idx[k];
            const abamd_row_meta_t pm = meta[p];
            int e = pm.end < qlen ? pm.end : qlen;
            const S *pH = arena + pm.off * 3;
            int32_t sc = (e >= pm.beg) ? (int32_t)pH[e - pm.beg] : jb.inf_min;
            if (sc > best_score) { best_score = sc; best_i = p; best_j = e; }
        }
    }
    if (tid == 0) {
        res->best_score = best_score;
        res->best_i = best_i; res->best_j = best_j;
    }
    if (!jb.ret_cigar) return;

    /* ---- backtrack (simd_abpoa_cg_backtrack transcription) ----
     * Thread 0 walks; the F planes are not stored, so when the insertion
     * branch needs F values the walk pauses and the whole block recomputes
     * the row's F window from the STORED (post-F) H plane:
     *   F'[rb] = inf_min - oe;  F'[j] = max(F'[j-1] - e, H[j-1] - oe)
     * — every backtrack decision is identical to stored-F (validated over
     * ~2.5M entries incl. entry-direction flips, tools/f_recompute_experiment.py,
     * and end-to-end by the parity suite). The window scan reuses the
     * per-wave local-scan + cross-wave-carry machinery of the forward pass
     * (same associativity/headroom argument). */
    __shared__ int bt_go, bt_bi_s, bt_bj_s;
    /* the F window aliases the row ring, dead since the barrier above */
    S *fbuf = &ring_lds[0][0];
    /* walk state: only thread 0's copies advance */
    int bi = best_i, bj = best_j, start_i = best_i, start_j = best_j;
    int cur_op = 0x1f, n_c = 0, status = ABAMD_JOB_OK;
    int look_end = jb.put_gap_at_end, put_right = jb.put_gap_on_right;
    int n_aln = 0, n_matched = 0;
    uint64_t *cig = jb.cigar;
    int id = jb.row_node_id[bi];
    int f_row = -1, f_wl = 0, f_hi = -1;
    if (tid == 0) {
        bt_go = 1;
        if (best_j < qlen) dev_push_cigar(cig, &n_c, jb.cigar_cap, 1, qlen - best_j, -1, qlen - 1, &status);
    }
    for (;;) {
        __syncthreads();
        if (bt_go == 0) break;
        if (bt_go == 2) {
            /* recompute F for row bt_bi_s, window ending at bt_bj_s */
            const int rbi = bt_bi_s;
            const abamd_row_meta_t bm = meta[rbi];
            const int rb = bm.beg, re = bm.end;
            const int hi = bt_bj_s < re ? bt_bj_s : re;
            const int wl = (hi - (BMW - 2)) > rb ? hi - (BMW - 2) : rb;
            const S *Hrow = arena + bm.off * 3;
            S carry1 = inf_min, carry2 = inf_min; /* F' at position ss-1 */
            for (int ss = rb; ss <= hi; ss += MWT) {
                const int j = ss + tid;
                const bool act2 = j <= hi;
                S c1, c2;
                if (!act2) { c1 = inf_min; c2 = inf_min; }
                else if (j == rb) { c1 = (S)(inf_min - oe1); c2 = (S)(inf_min - oe2); }
                else {
                    const S hp = Hrow[j - 1 - rb];
                    c1 = (S)(hp - oe1);
                    c2 = (S)(hp - oe2);
                }
                S L1 = scan_maxplus(c1, jb.e1, inf_min, lane);
                S L2 = scan_maxplus(c2, jb.e2, inf_min, lane);
                if (lane == WAVE - 1) { sc_f1[wv] = L1; sc_f2[wv] = L2; }
                __syncthreads();
                /* F' entering this wave; no carry exists before the band
                 * start (mirrors the forward pass: wave 0 of the first
                 * superchunk takes its local scan verbatim) */
                S C1 = carry1, C2 = carry2;
                bool havec = ss != rb;
                for (int ww = 0; ww < wv; ++ww) {
                    if (havec) {
                        C1 = smax(sc_f1[ww], (S)(C1 - (S)(WAVE * jb.e1)));
                        C2 = smax(sc_f2[ww], (S)(C2 - (S)(WAVE * jb.e2)));
                    } else {
                        C1 = sc_f1[ww]; C2 = sc_f2[ww];
                        havec = true;
                    }
                }
                S f1 = L1, f2 = L2;
                if (havec) {
                    f1 = smax(L1, (S)(C1 - (S)((lane + 1) * jb.e1)));
                    f2 = smax(L2, (S)(C2 - (S)((lane + 1) * jb.e2)));
                }
                if (act2 && j >= wl) {
                    fbuf[j - wl] = f1;
                    fbuf[BMW + j - wl] = f2;
                }
                const bool more2 = ss + MWT <= hi;
                if (more2 && j == ss + MWT - 1) { sc_carry[0] = f1; sc_carry[1] = f2; }
                __syncthreads();
                if (more2) { carry1 = sc_carry[0]; carry2 = sc_carry[1]; }
            }
            f_row = rbi; f_wl = wl; f_hi = hi;
            __syncthreads();
        }
        if (tid == 0) {
            int pause = 0;
            while (bi > 0 && bj > 0 && status == ABAMD_JOB_OK) {
                const abamd_row_meta_t bm = meta[bi];
                const int rb = bm.beg, re = bm.end;
                const int64_t bw = re - rb + 1;
                const S *H = arena + bm.off * 3;
                const S *E1r = H + bw, *E2r = E1r + bw;
                const S Hj = (bj >= rb && bj <= re) ? H[bj - rb] : inf_min;
                const S Hjm1 = (bj - 1 >= rb && bj - 1 <= re) ? H[bj - 1 - rb] : inf_min;
                const S E1j = (bj >= rb && bj <= re) ? E1r[bj - rb] : inf_min;
                const S E2j = (bj >= rb && bj <= re) ? E2r[bj - rb] : inf_min;
                if (local_mode && Hj == 0) break;
                start_i = bi; start_j = bj;
                const int pq0 = jb.pre_off[bi], pq1 = jb.pre_off[bi + 1];
                const S s = (S)mat_lds[m * jb.row_base[bi] + query[bj - 1]];
                const int is_match = jb.row_base[bi] == query[bj - 1];
                int hit = 0;
                if (put_right == 0 && look_end == 0 && (cur_op & 0x1)) {
                    for (int k = pq0; k < pq1; ++k) {
                        const int p = jb.pre_idx[k];
                        const S ps = (S)jb.pre_ps[k];
                        const abamd_row_meta_t pm = meta[p];
                        if (bj - 1 < pm.beg || bj - 1 > pm.end) continue;
                        const S *pH = arena + pm.off * 3;
                        if ((S)(pH[bj - 1 - pm.beg] + s + ps) == Hj) {
                            dev_push_cigar(cig, &n_c, jb.cigar_cap, 0, 1, id, bj - 1, &status);
                            bi = p; --bj; id = jb.row_node_id[bi]; hit = 1;
                            cur_op = 0x1f; ++n_aln; n_matched += is_match;
                            break;
                        }
                    }
                }
                if (!hit && (cur_op & 0x6)) { /* deletion */
                    for (int k = pq0; k < pq1; ++k) {
                        const int p = jb.pre_idx[k];
                        const S ps = (S)jb.pre_ps[k];
                        const abamd_row_meta_t pm = meta[p];
                        if (bj < pm.beg || bj > pm.end) continue;
                        const int poffc = bj - pm.beg;
                        const int64_t pbw = pm.end - pm.beg + 1;
                        const S *pH = arena + pm.off * 3;
                        const S *pE1 = pH + pbw, *pE2 = pE1 + pbw;
                        if (cur_op & 0x2) {
                            if (cur_op & 0x1) {
                                if (Hj == (S)(pE1[poffc] + ps)) {
                                    cur_op = ((S)(pH[poffc] - oe1) == pE1[poffc]) ? (0x1 | 0x18) : 0x2;
                                    hit = 1; dev_push_cigar(cig, &n_c, jb.cigar_cap, 2, 1, id, bj - 1, &status);
                                    bi = p; id = jb.row_node_id[bi];
                                    if (look_end) look_end = 0;
                                    break;
                                }
                            } else {
                                if (E1j == (S)(pE1[poffc] - e1 + ps)) {
                                    cur_op = ((S)(pH[poffc] - oe1) == pE1[poffc]) ? (0x1 | 0x18) : 0x2;
                                    hit = 1; dev_push_cigar(cig, &n_c, jb.cigar_cap, 2, 1, id, bj - 1, &status);
                                    bi = p; id = jb.row_node_id[bi];
                                    if (look_end) look_end = 0;
                                    break;
                                }
                            }
                        }
                        if (cur_op & 0x4) {
                            if (cur_op & 0x1) {
                                if (Hj == (S)(pE2[poffc] + ps)) {
                                    cur_op = ((S)(pH[poffc] - oe2) == pE2[poffc]) ? (0x1 | 0x18) : 0x4;
                                    hit = 1; dev_push_cigar(cig, &n_c, jb.cigar_cap, 2, 1, id, bj - 1, &status);
                                    bi = p; id = jb.row_node_id[bi];
                                    if (look_end) look_end = 0;
                                    break;
                                }
                            } else {
                                if (E2j == (S)(pE2[poffc] - e2 + ps)) {
                                    cur_op = ((S)(pH[poffc] - oe2) == pE2[poffc]) ? (0x1 | 0x18) : 0x4;
                                    hit = 1; dev_push_cigar(cig, &n_c, jb.cigar_cap, 2, 1, id, bj - 1, &status);
                                    bi = p; id = jb.row_node_id[bi];
                                    if (look_end) look_end = 0;
                                    break;
                                }
                            }
                        }
                    }
                }
                if (!hit && (cur_op & 0x18)) { /* insertion: needs recomputed F */
                    const bool needj = (bj >= rb && bj <= re);
                    const bool needj1 = (bj - 1 >= rb && bj - 1 <= re);
                    const bool cover = (f_row == bi)
                        && (!needj || (bj >= f_wl && bj <= f_hi))
                        && (!needj1 || (bj - 1 >= f_wl && bj - 1 <= f_hi));
                    if ((needj || needj1) && !cover) {
                        bt_bi_s = bi; bt_bj_s = bj; bt_go = 2;
                        pause = 1;
                        break; /* re-enter this step after the block recomputes */
                    }
                    const S F1j = needj ? fbuf[bj - f_wl] : inf_min;
                    const S F2j = needj ? fbuf[BMW + bj - f_wl] : inf_min;
                    const S F1jm1 = needj1 ? fbuf[bj - 1 - f_wl] : inf_min;
                    const S F2jm1 = needj1 ? fbuf[BMW + bj - 1 - f_wl] : inf_min;
                    if (cur_op & 0x8) {
                        if (cur_op & 0x1) {
                            if (Hj == F1j) {
                                if ((S)(Hjm1 - oe1) == F1j) { cur_op = 0x1 | 0x6; hit = 1; }
                                else if ((S)(F1jm1 - e1) == F1j) { cur_op = 0x8; hit = 1; }
                            }
                        } else {
                            if ((S)(Hjm1 - oe1) == F1j) { cur_op = 0x1 | 0x6; hit = 1; }
                            else if ((S)(F1jm1 - e1) == F1j) { cur_op = 0x8; hit = 1; }
                        }
                    }
                    if (!hit && (cur_op & 0x10)) {
                        if (cur_op & 0x1) {
                            if (Hj == F2j) {
                                if ((S)(Hjm1 - oe2) == F2j) { cur_op = 0x1 | 0x6; hit = 1; }
                                else if ((S)(F2jm1 - e2) == F2j) { cur_op = 0x10; hit = 1; }
                            }
                        } else {
                            if ((S)(Hjm1 - oe2) == F2j) { cur_op = 0x1 | 0x6; hit = 1; }
                            else if ((S)(F2jm1 - e2) == F2j) { cur_op = 0x10; hit = 1; }
                        }
                    }
                    if (hit) {
                        dev_push_cigar(cig, &n_c, jb.cigar_cap, 1, 1, id, bj - 1, &status);
                        --bj;
                        if (look_end) look_end = 0;
                        ++n_aln;
                    }
                }
                if (!hit && (cur_op & 0x1)) {
                    for (int k = pq0; k < pq1; ++k) {
                        const int p = jb.pre_idx[k];
                        const S ps = (S)jb.pre_ps[k];
                        const abamd_row_meta_t pm = meta[p];
                        if (bj - 1 < pm.beg || bj - 1 > pm.end) continue;
                        const S *pH = arena + pm.off * 3;
                        if ((S)(pH[bj - 1 - pm.beg] + s + ps) == Hj) {
                            dev_push_cigar(cig, &n_c, jb.cigar_cap, 0, 1, id, bj - 1, &status);
                            bi = p; --bj; id = jb.row_node_id[bi]; hit = 1;
                            cur_op = 0x1f; ++n_aln; n_matched += is_match;
                            look_end = 0;
                            break;
                        }
                    }
                }
                if (!hit) { status = ABAMD_JOB_BT_DEAD_END; break; }
            }
            if (!pause) {
                if (status == ABAMD_JOB_OK && bj > 0)
                    dev_push_cigar(cig, &n_c, jb.cigar_cap, 1, bj, -1, bj - 1, &status);
                res->status = status;
                res->n_cigar = n_c;
                res->n_aln_bases = n_aln;
                res->n_matched_bases = n_matched;
                res->node_e = jb.row_node_id[best_i]; res->query_e = best_j - 1;
                res->node_s = jb.row_node_id[start_i]; res->query_s = start_j - 1;
                bt_go = 0;
            }
        }
    }
}

extern "C" int abamd_dp_ring_depth(void) {
    /* read per call (one getenv per job build): tests flip it in-process */
    const char *e = getenv("ABPOA_AMD_DP_RING");
    int d = (e && *e) ? atoi(e) : ABAMD_DP_RING_MAX;
    if (d < 1) d = 1;
    if (d > ABAMD_DP_RING_MAX) d = ABAMD_DP_RING_MAX;
    return d;
}

extern "C" int abamd_dp_force_generic(void) {
    /* read per call, like the ring depth */
    const char *e = getenv("ABPOA_AMD_DP_GENERIC");
    return e && *e && atoi(e) != 0;
}

extern "C" int abamd_cg_fast_eligible(int align_mode, int banded, int inc_path_score, int dp_ring) {
    return align_mode == 0 && banded && !inc_path_score && dp_ring == ABAMD_DP_RING_MAX;
}

extern "C" void abamd_launch_cg_i16(const abamd_gpu_job_t *dev_jobs, abamd_gpu_res_t *dev_res,
                                    int n_jobs, int fast, void *stream) {
    if (fast)
        hipLaunchKernelGGL((cg_global_mw_kernel<int16_t, true>), dim3(n_jobs), dim3(MWT), 0,
                           (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
    else
        hipLaunchKernelGGL((cg_global_mw_kernel<int16_t, false>), dim3(n_jobs), dim3(MWT), 0,
                           (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
}
extern "C" void abamd_launch_cg_i32(const abamd_gpu_job_t *dev_jobs, abamd_gpu_res_t *dev_res,
                                    int n_jobs, int fast, void *stream) {
    if (fast)
        hipLaunchKernelGGL((cg_global_mw_kernel<int32_t, true>), dim3(n_jobs), dim3(MWT), 0,
                           (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
    else
        hipLaunchKernelGGL((cg_global_mw_kernel<int32_t, false>), dim3(n_jobs), dim3(MWT), 0,
                           (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
}

/* ------------------------------------------------------------------ */
/* Multi-wave affine kernel (3 planes H,E1,F1): same 8-waves-per-job   */
/* design as the convex kernel; the F chain feeds from H BEFORE the E  */
/* fold (simd_abpoa_ag_dp, abpoa_align_simd.c:817-933) and the stored  */
/* E is inf_min when the insertion won the cell (SIMDSetIfEqual, :930).*/
/* The H and E1 bands of the previous row stay in a double-buffered    */
/* LDS cache; other predecessors, and rows wider than BMW, are read    */
/* from the arena.                                                      */
/* ------------------------------------------------------------------ */
template <typename S>
__global__ __launch_bounds__(MWT, 1)
void ag_global_mw_kernel(const abamd_gpu_job_t *__restrict__ jobs,
                         abamd_gpu_res_t *__restrict__ results, int n_jobs) {
    const int jid = blockIdx.x;
    if (jid >= n_jobs) return;
    const int tid = threadIdx.x;
    const int wv = tid / WAVE, lane = tid % WAVE;

    __shared__ int mat_lds[27 * 27];
    __shared__ S prev_lds[2][2 * BMW];
    __shared__ S sc_h[MWAVES], sc_f1[MWAVES];
    __shared__ int sc_red[3 * MWAVES];
    __shared__ S sc_carry[2];

    /* by VALUE: every field lives in registers (uniform loads become
       s_loads into SGPRs) — a reference would re-load fields from global
       memory inside the row loop because arena/steering stores could alias
       the jobs array in the compiler's view */
    const abamd_gpu_job_t jb = jobs[jid];
    abamd_gpu_res_t *res = &results[jid];
    abamd_row_meta_t *__restrict__ meta = (abamd_row_meta_t*)jb.row_meta;

    const int n_rows = jb.n_rows, m = jb.m;
    const S inf_min = (S)jb.inf_min;
    const S e1 = (S)jb.e1, oe1 = (S)jb.oe1;
    const int local_mode = jb.align_mode == 1;
    mw_best_t run = { jb.inf_min, 0, 0, jb.max_remain[0], 0 };
    const int end_remain = jb.max_remain[n_rows - 1];
    S *arena = (S*)jb.arena;
    const uint8_t *__restrict__ query = jb.query;

    for (int i = tid; i < m * m; i += MWT) mat_lds[i] = jb.mat[i];
    if (tid == 0) { res->status = ABAMD_JOB_OK; res->n_cigar = 0; }
    mw_steer_init(jb, tid);
    __syncthreads();

    int buf_cur = 0;
    mw_prev_t prev = { 0, -1, 0, -1 };

    /* first row (simd_abpoa_ag_first_dp, abpoa_align_simd.c:651-667) */
    int64_t used;
    {
        const int end0 = mw_first_row_end(jb, end_remain);
        if (tid == 0) { meta[0].beg = 0; meta[0].end = end0; meta[0].off = 0; }
        int64_t bw = end0 + 1;
        used = bw;
        S *H = arena, *E1 = arena + bw, *F1 = arena + 2 * bw;
        S *c = &prev_lds[buf_cur][0];
        const int fits = end0 + 1 <= BMW;
        for (int j = tid; j <= end0; j += MWT) {
            S hv, e1v2;
            if (local_mode) {
                hv = 0; e1v2 = 0; F1[j] = 0;
            } else if (j == 0) {
                hv = 0; e1v2 = (S)(0 - oe1);
                F1[0] = inf_min;
            } else {
                S f1 = (S)(-(jb.o1 + jb.e1 * j));
                F1[j] = f1;
                hv = f1; e1v2 = inf_min;
            }
            H[j] = hv; E1[j] = e1v2;
            if (fits) { c[j] = hv; c[BMW + j] = e1v2; }
        }
        if (fits) prev = mw_prev_t{ 1, 0, 0, end0 };
        buf_cur ^= 1;
        __syncthreads();
    }

    const bool rowmax = mw_needs_rowmax(jb);
    mw_row_t nxt;
    nxt.first(jb);
    for (int r = 1; r < n_rows - 1; ++r) {
        const mw_row_t row = nxt;
        nxt.advance(jb, r + 1);
        const int pk0 = row.pk0, pk1 = row.pk1;
        const S ps0 = (S)row.ps0;
        int beg, end;
        mw_row_band(jb, meta, row, prev, end_remain, beg, end);
        const int64_t bw = end - beg + 1;
        const int64_t off = mw_row_reserve(jb, meta, tid, r, beg, end, used);
        if (off < 0) { if (tid == 0) res->status = ABAMD_JOB_ARENA_OVERFLOW; return; }
        S *H = arena + off * 3, *E1r = H + bw, *F1r = E1r + bw;
        const uint8_t base = jb.row_base[r];
        const int *mrow = &mat_lds[base * m];
        const int cache_fits = bw <= BMW;
        S *cw = &prev_lds[buf_cur][0];
        const S *cr = &prev_lds[buf_cur ^ 1][0];
        const bool fast1 = (pk1 - pk0 == 1) && prev.ok && (row.pidx0 == prev.row);

        S carry_hm = inf_min, f1c = inf_min;
        S lmax = inf_min; int lleft = -1, lright = -1;

        for (int ss = beg; ss <= end; ss += MWT) {
            const int j = ss + tid;
            const bool act = j <= end;
            S h = inf_min, e1v = inf_min;
            if (fast1) {
                if (act) {
                    if (local_mode && j == 0) { if (ps0 > h) h = ps0; }
                    if (j - 1 >= prev.beg && j - 1 <= prev.end) {
                        S v = (S)(cr[j - 1 - prev.beg] + ps0);
                        if (v > h) h = v;
                    }
                    if (j >= prev.beg && j <= prev.end) {
                        S v1 = (S)(cr[BMW + j - prev.beg] + ps0);
                        if (v1 > e1v) e1v = v1;
                    }
                }
            } else for (int k = pk0; k < pk1; ++k) {
                const int p = jb.pre_idx[k];
                const S ps = (S)jb.pre_ps[k];
                if (prev.ok && p == prev.row) {
                    if (act) {
                        if (local_mode && j == 0) { if (ps > h) h = ps; }
                        if (j - 1 >= prev.beg && j - 1 <= prev.end) {
                            S v = (S)(cr[j - 1 - prev.beg] + ps);
                            if (v > h) h = v;
                        }
                        if (j >= prev.beg && j <= prev.end) {
                            S v1 = (S)(cr[BMW + j - prev.beg] + ps);
                            if (v1 > e1v) e1v = v1;
                        }
                    }
                    continue;
                }
                const abamd_row_meta_t pm = meta[p];
                const int64_t pbw = pm.end - pm.beg + 1;
                const S *__restrict__ pH = arena + pm.off * 3;
                const S *__restrict__ pE1 = pH + pbw;
                if (act) {
                    if (local_mode && j == 0) { if (ps > h) h = ps; }
                    if (j - 1 >= pm.beg && j - 1 <= pm.end) {
                        S v = (S)(pH[j - 1 - pm.beg] + ps);
                        if (v > h) h = v;
                    }
                    if (j >= pm.beg && j <= pm.end) {
                        S v1 = (S)(pE1[j - pm.beg] + ps);
                        if (v1 > e1v) e1v = v1;
                    }
                }
            }
            const S q = (S)((j == 0 || !act) ? 0 : mrow[query[j - 1]]);
            S hm = (S)(h + q);   /* M+q: the F chain feeds from this, pre-E */
            if (!act) hm = inf_min;

            if (lane == WAVE - 1) sc_h[wv] = hm;
            __syncthreads(); /* wave edges of hm */
            S hmshift = (S)__shfl_up((int)hm, 1);
            S c1;
            if (lane == 0) {
                if (wv == 0) {
                    if (ss == beg) c1 = (S)(inf_min - oe1);
                    else c1 = smax((S)(carry_hm - oe1), (S)(f1c - e1));
                } else {
                    c1 = (S)(sc_h[wv - 1] - oe1);
                }
            } else c1 = (S)(hmshift - oe1);
            S L1 = scan_maxplus(c1, jb.e1, inf_min, lane);
            if (lane == WAVE - 1) sc_f1[wv] = L1;
            __syncthreads(); /* per-wave local scans */
            S f1 = L1;
            if (wv > 0) {
                S C1 = sc_f1[0];
                for (int ww = 1; ww < wv; ++ww)
                    C1 = smax(sc_f1[ww], (S)(C1 - (S)(WAVE * jb.e1)));
                f1 = smax(L1, (S)(C1 - (S)((lane + 1) * jb.e1)));
            }

            S tmp = smax(hm, e1v);
            S hf = smax(tmp, f1);
            if (local_mode) hf = smax(hf, (S)0);
            S e1n = (hf == tmp) ? smax((S)(e1v - e1), (S)(hf - oe1))
                                : (local_mode ? (S)0 : inf_min);
            if (act) {
                H[j - beg] = hf; E1r[j - beg] = e1n; F1r[j - beg] = f1;
                if (cache_fits) { cw[j - beg] = hf; cw[BMW + j - beg] = e1n; }
                if (hf > lmax) { lmax = hf; lleft = j; lright = j; }
                else if (hf == lmax) { lright = j; }
            }
            const bool more = ss + MWT <= end;
            if (more && j == ss + MWT - 1) {
                sc_carry[0] = hm; sc_carry[1] = f1;
            }
            if (!more && rowmax)
                mw_rowmax_publish(sc_red, wv, lane, lmax, lleft, lright);
            __syncthreads(); /* also orders cw writes before the next row's reads */
            if (more) { carry_hm = sc_carry[0]; f1c = sc_carry[1]; }
        }

        if (cache_fits) prev = mw_prev_t{ 1, r, beg, end };
        else prev.ok = 0;
        buf_cur ^= 1;

        if (mw_row_close(jb, sc_red, row, r, run, nxt)) break;
    }

    __syncthreads();
    if (tid == 0) res->cells = used;
    if (tid != 0) return;

    int32_t best_score;
    int best_i, best_j;
    mw_final_best<S>(jb, run, 3, best_score, best_i, best_j);
    res->best_score = best_score;
    res->best_i = best_i; res->best_j = best_j;
    if (!jb.ret_cigar) return;

    /* simd_abpoa_ag_backtrack (:196-307) */
    mw_walk_t wk = mw_walk_begin(jb, best_i, best_j);
    int cur_op = 0x1f;
    while (wk.bi > 0 && wk.bj > 0 && wk.status == ABAMD_JOB_OK) {
        const int bi = wk.bi, bj = wk.bj; /* the cell this step leaves */
        const abamd_row_meta_t bm = meta[bi];
        const int rb = bm.beg, re = bm.end;
        const int64_t bw = re - rb + 1;
        const S *H = arena + bm.off * 3;
        const S *E1r = H + bw, *F1r = E1r + bw;
        const S Hj = (bj >= rb && bj <= re) ? H[bj - rb] : inf_min;
        const S Hjm1 = (bj - 1 >= rb && bj - 1 <= re) ? H[bj - 1 - rb] : inf_min;
        const S E1j = (bj >= rb && bj <= re) ? E1r[bj - rb] : inf_min;
        const S F1j = (bj >= rb && bj <= re) ? F1r[bj - rb] : inf_min;
        const S F1jm1 = (bj - 1 >= rb && bj - 1 <= re) ? F1r[bj - 1 - rb] : inf_min;
        if (local_mode && Hj == 0) break;
        wk.start_i = bi; wk.start_j = bj;
        const int pq0 = jb.pre_off[bi], pq1 = jb.pre_off[bi + 1];
        const S s = (S)mat_lds[m * jb.row_base[bi] + query[bj - 1]];
        const int is_match = jb.row_base[bi] == query[bj - 1];
        int hit = 0;
        if (wk.put_right == 0 && wk.look_end == 0 && (cur_op & 0x1)) {
            hit = mw_walk_match<S>(jb, wk, 3, pq0, pq1, s, is_match, Hj);
            if (hit) cur_op = 0x1f;
        }
        if (!hit && (cur_op & 0x2)) { /* deletion: entered from H, or E extended */
            for (int k = pq0; k < pq1; ++k) {
                const int p = jb.pre_idx[k];
                const S ps = (S)jb.pre_ps[k];
                const abamd_row_meta_t pm = meta[p];
                if (bj < pm.beg || bj > pm.end) continue;
                const int poffc = bj - pm.beg;
                const int64_t pbw = pm.end - pm.beg + 1;
                const S *pH = arena + pm.off * 3;
                const S *pE1 = pH + pbw;
                if ((cur_op & 0x1) ? Hj == (S)(pE1[poffc] + ps)
                                   : E1j == (S)(pE1[poffc] - e1 + ps)) {
                    cur_op = ((S)(pH[poffc] - oe1) == pE1[poffc]) ? (0x1 | 0x18) : 0x2;
                    hit = 1;
                    dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 2, 1, wk.id, bj - 1, &wk.status);
                    wk.bi = p; wk.id = jb.row_node_id[p];
                    wk.look_end = 0;
                    break;
                }
            }
        }
        if (!hit && (cur_op & 0x18)) { /* insertion */
            if (!(cur_op & 0x1) || Hj == F1j) {
                if ((S)(Hjm1 - oe1) == F1j) { cur_op = 0x1 | 0x6; hit = 1; }
                else if ((S)(F1jm1 - e1) == F1j) { cur_op = 0x8; hit = 1; }
            }
            if (hit) {
                dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 1, 1, wk.id, bj - 1, &wk.status);
                --wk.bj;
                wk.look_end = 0;
                ++wk.n_aln;
            }
        }
        if (!hit && (cur_op & 0x1)) {
            hit = mw_walk_match<S>(jb, wk, 3, pq0, pq1, s, is_match, Hj);
            if (hit) { cur_op = 0x1f; wk.look_end = 0; }
        }
        if (!hit) { wk.status = ABAMD_JOB_BT_DEAD_END; break; }
    }
    mw_walk_end(jb, res, wk, best_i, best_j);
}

/* ------------------------------------------------------------------ */
/* Multi-wave linear kernel (1 plane): candidates carry the query score */
/* and the deletion term, then the insertion max-plus scan runs on H    */
/* itself (simd_abpoa_lg_dp, abpoa_align_simd.c:727-815). The local     */
/* clamp applies AFTER the scan, and every carry (between waves and     */
/* between superchunks) is the PRE-clamp scan value: the reference      */
/* clamps a row only once its whole insertion chain has run (:814).     */
/* ------------------------------------------------------------------ */
template <typename S>
__global__ __launch_bounds__(MWT, 1)
void lg_global_mw_kernel(const abamd_gpu_job_t *__restrict__ jobs,
                         abamd_gpu_res_t *__restrict__ results, int n_jobs) {
    const int jid = blockIdx.x;
    if (jid >= n_jobs) return;
    const int tid = threadIdx.x;
    const int wv = tid / WAVE, lane = tid % WAVE;

    __shared__ int mat_lds[27 * 27];
    __shared__ S prev_lds[2][BMW];
    __shared__ S sc_f1[MWAVES];
    __shared__ int sc_red[3 * MWAVES];
    __shared__ S sc_carry[1];

    /* by VALUE, for the reason given in the affine kernel */
    const abamd_gpu_job_t jb = jobs[jid];
    abamd_gpu_res_t *res = &results[jid];
    abamd_row_meta_t *__restrict__ meta = (abamd_row_meta_t*)jb.row_meta;

    const int n_rows = jb.n_rows, m = jb.m;
    const S inf_min = (S)jb.inf_min;
    const S e1 = (S)jb.e1;
    const int local_mode = jb.align_mode == 1;
    mw_best_t run = { jb.inf_min, 0, 0, jb.max_remain[0], 0 };
    const int end_remain = jb.max_remain[n_rows - 1];
    S *arena = (S*)jb.arena;
    const uint8_t *__restrict__ query = jb.query;

    for (int i = tid; i < m * m; i += MWT) mat_lds[i] = jb.mat[i];
    if (tid == 0) { res->status = ABAMD_JOB_OK; res->n_cigar = 0; }
    mw_steer_init(jb, tid);
    __syncthreads();

    int buf_cur = 0;
    mw_prev_t prev = { 0, -1, 0, -1 };

    /* first row (simd_abpoa_lg_first_dp, abpoa_align_simd.c:635-649) */
    int64_t used;
    {
        const int end0 = mw_first_row_end(jb, end_remain);
        if (tid == 0) { meta[0].beg = 0; meta[0].end = end0; meta[0].off = 0; }
        used = end0 + 1;
        S *H = arena;
        S *c = &prev_lds[buf_cur][0];
        const int fits = end0 + 1 <= BMW;
        for (int j = tid; j <= end0; j += MWT) {
            S hv = local_mode ? (S)0 : (S)(-jb.e1 * j);
            H[j] = hv;
            if (fits) c[j] = hv;
        }
        if (fits) prev = mw_prev_t{ 1, 0, 0, end0 };
        buf_cur ^= 1;
        __syncthreads();
    }

    const bool rowmax = mw_needs_rowmax(jb);
    mw_row_t nxt;
    nxt.first(jb);
    for (int r = 1; r < n_rows - 1; ++r) {
        const mw_row_t row = nxt;
        nxt.advance(jb, r + 1);
        const int pk0 = row.pk0, pk1 = row.pk1;
        const S ps0 = (S)row.ps0;
        int beg, end;
        mw_row_band(jb, meta, row, prev, end_remain, beg, end);
        const int64_t bw = end - beg + 1;
        const int64_t off = mw_row_reserve(jb, meta, tid, r, beg, end, used);
        if (off < 0) { if (tid == 0) res->status = ABAMD_JOB_ARENA_OVERFLOW; return; }
        S *H = arena + off;
        const uint8_t base = jb.row_base[r];
        const int *mrow = &mat_lds[base * m];
        const int cache_fits = bw <= BMW;
        S *cw = &prev_lds[buf_cur][0];
        const S *cr = &prev_lds[buf_cur ^ 1][0];
        const bool fast1 = (pk1 - pk0 == 1) && prev.ok && (row.pidx0 == prev.row);

        S carry_h = inf_min;                 /* PRE-clamp scan value at ss-1 */
        S lmax = inf_min; int lleft = -1, lright = -1;

        for (int ss = beg; ss <= end; ss += MWT) {
            const int j = ss + tid;
            const bool act = j <= end;
            const S q = (S)((j == 0 || !act) ? 0 : mrow[query[j - 1]]);
            S h = inf_min;
            if (fast1) {
                if (act) {
                    if (local_mode && j == 0) { S v = (S)(ps0 + q); if (v > h) h = v; }
                    if (j - 1 >= prev.beg && j - 1 <= prev.end) {
                        S v = (S)(cr[j - 1 - prev.beg] + ps0 + q);
                        if (v > h) h = v;
                    }
                    if (j >= prev.beg && j <= prev.end) {
                        S v = (S)(cr[j - prev.beg] + ps0 - e1);
                        if (v > h) h = v;
                    }
                }
            } else for (int k = pk0; k < pk1; ++k) {
                const int p = jb.pre_idx[k];
                const S ps = (S)jb.pre_ps[k];
                if (prev.ok && p == prev.row) {
                    if (act) {
                        if (local_mode && j == 0) { S v = (S)(ps + q); if (v > h) h = v; }
                        if (j - 1 >= prev.beg && j - 1 <= prev.end) {
                            S v = (S)(cr[j - 1 - prev.beg] + ps + q);
                            if (v > h) h = v;
                        }
                        if (j >= prev.beg && j <= prev.end) {
                            S v = (S)(cr[j - prev.beg] + ps - e1);
                            if (v > h) h = v;
                        }
                    }
                    continue;
                }
                const abamd_row_meta_t pm = meta[p];
                const S *__restrict__ pH = arena + pm.off;
                if (act) {
                    if (local_mode && j == 0) { S v = (S)(ps + q); if (v > h) h = v; }
                    if (j - 1 >= pm.beg && j - 1 <= pm.end) {
                        S v = (S)(pH[j - 1 - pm.beg] + ps + q);
                        if (v > h) h = v;
                    }
                    if (j >= pm.beg && j <= pm.end) {
                        S v = (S)(pH[j - pm.beg] + ps - e1);
                        if (v > h) h = v;
                    }
                }
            }
            if (!act) h = inf_min;

            /* insertion scan ON H: per-wave local scan + cross-wave carry.
             * Splitting the row's one max-plus chain at the wave edges is
             * exact: the decays regroup under wrapping arithmetic. */
            S L1 = scan_maxplus(h, jb.e1, inf_min, lane);
            if (lane == WAVE - 1) sc_f1[wv] = L1;
            __syncthreads(); /* per-wave local scans */
            S hsc = L1;
            {
                S C1 = carry_h;
                bool havec = ss != beg;
                for (int ww = 0; ww < wv; ++ww) {
                    if (havec) C1 = smax(sc_f1[ww], (S)(C1 - (S)(WAVE * jb.e1)));
                    else { C1 = sc_f1[ww]; havec = true; }
                }
                if (havec) hsc = smax(L1, (S)(C1 - (S)((lane + 1) * jb.e1)));
            }
            S hfin = local_mode ? smax(hsc, (S)0) : hsc; /* clamp AFTER scan+carry */
            if (act) {
                H[j - beg] = hfin;
                if (cache_fits) cw[j - beg] = hfin;
                if (hfin > lmax) { lmax = hfin; lleft = j; lright = j; }
                else if (hfin == lmax) { lright = j; }
            }
            const bool more = ss + MWT <= end;
            if (more && j == ss + MWT - 1) sc_carry[0] = hsc; /* PRE-clamp */
            if (!more && rowmax)
                mw_rowmax_publish(sc_red, wv, lane, lmax, lleft, lright);
            __syncthreads(); /* also orders cw writes before the next row's reads */
            if (more) carry_h = sc_carry[0];
        }

        if (cache_fits) prev = mw_prev_t{ 1, r, beg, end };
        else prev.ok = 0;
        buf_cur ^= 1;

        if (mw_row_close(jb, sc_red, row, r, run, nxt)) break;
    }

    __syncthreads();
    if (tid == 0) res->cells = used;
    if (tid != 0) return;

    int32_t best_score;
    int best_i, best_j;
    mw_final_best<S>(jb, run, 1, best_score, best_i, best_j);
    res->best_score = best_score;
    res->best_i = best_i; res->best_j = best_j;
    if (!jb.ret_cigar) return;

    /* simd_abpoa_lg_backtrack (:116-194) */
    mw_walk_t wk = mw_walk_begin(jb, best_i, best_j);
    while (wk.bi > 0 && wk.bj > 0 && wk.status == ABAMD_JOB_OK) {
        const int bi = wk.bi, bj = wk.bj; /* the cell this step leaves */
        const abamd_row_meta_t bm = meta[bi];
        const int rb = bm.beg, re = bm.end;
        const S *H = arena + bm.off;
        const S Hj = (bj >= rb && bj <= re) ? H[bj - rb] : inf_min;
        const S Hjm1 = (bj - 1 >= rb && bj - 1 <= re) ? H[bj - 1 - rb] : inf_min;
        if (local_mode && Hj == 0) break;
        wk.start_i = bi; wk.start_j = bj;
        const int pq0 = jb.pre_off[bi], pq1 = jb.pre_off[bi + 1];
        const S s = (S)mat_lds[m * jb.row_base[bi] + query[bj - 1]];
        const int is_match = jb.row_base[bi] == query[bj - 1];
        int hit = 0;
        if (wk.put_right == 0 && wk.look_end == 0)
            hit = mw_walk_match<S>(jb, wk, 1, pq0, pq1, s, is_match, Hj);
        if (!hit) { /* deletion */
            for (int k = pq0; k < pq1; ++k) {
                const int p = jb.pre_idx[k];
                const S ps = (S)jb.pre_ps[k];
                const abamd_row_meta_t pm = meta[p];
                if (bj < pm.beg || bj > pm.end) continue;
                const S *pH = arena + pm.off;
                if ((S)(pH[bj - pm.beg] - e1 + ps) == Hj) {
                    dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 2, 1, wk.id, bj - 1, &wk.status);
                    wk.bi = p; wk.id = jb.row_node_id[p]; hit = 1;
                    wk.look_end = 0;
                    break;
                }
            }
        }
        if (!hit && (S)(Hjm1 - e1) == Hj) { /* insertion */
            dev_push_cigar(jb.cigar, &wk.n_c, jb.cigar_cap, 1, 1, wk.id, bj - 1, &wk.status);
            --wk.bj;
            wk.look_end = 0;
            hit = 1; ++wk.n_aln;
        }
        if (!hit) {
            hit = mw_walk_match<S>(jb, wk, 1, pq0, pq1, s, is_match, Hj);
            if (hit) wk.look_end = 0;
        }
        if (!hit) { wk.status = ABAMD_JOB_BT_DEAD_END; break; }
    }
    mw_walk_end(jb, res, wk, best_i, best_j);
}

extern "C" void abamd_launch_ag_i16(const abamd_gpu_job_t *dev_jobs, abamd_gpu_res_t *dev_res,
                                    int n_jobs, void *stream) {
    hipLaunchKernelGGL((ag_global_mw_kernel<int16_t>), dim3(n_jobs), dim3(MWT), 0,
                       (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
}
extern "C" void abamd_launch_ag_i32(const abamd_gpu_job_t *dev_jobs, abamd_gpu_res_t *dev_res,
                                    int n_jobs, void *stream) {
    hipLaunchKernelGGL((ag_global_mw_kernel<int32_t>), dim3(n_jobs), dim3(MWT), 0,
                       (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
}
extern "C" void abamd_launch_lg_i16(const abamd_gpu_job_t *dev_jobs, abamd_gpu_res_t *dev_res,
                                    int n_jobs, void *stream) {
    hipLaunchKernelGGL((lg_global_mw_kernel<int16_t>), dim3(n_jobs), dim3(MWT), 0,
                       (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
}
extern "C" void abamd_launch_lg_i32(const abamd_gpu_job_t *dev_jobs, abamd_gpu_res_t *dev_res,
                                    int n_jobs, void *stream) {
    hipLaunchKernelGGL((lg_global_mw_kernel<int32_t>), dim3(n_jobs), dim3(MWT), 0,
                       (hipStream_t)stream, dev_jobs, dev_res, n_jobs);
}

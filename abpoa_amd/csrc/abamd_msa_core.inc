/* abamd_msa_core.inc — shared host/device body for the row-column MSA over
 * the FLAT graph layout: the device-resident batch driver builds each set's
 * alignment matrix on the GPU after its last fold and downloads only the
 * matrix, instead of downloading the graph for abpoa_generate_rc_msa.
 *
 * Mirrors abpoa_generate_rc_msa (abamd_cons.c; reference abpoa_output.c
 * :106-148): the LIFO rank walk of dfs_set_msa_rank (abamd_graph.c) defines
 * the column order, a node's column is max(rank over the node and its aligned
 * group) - 1 (group_msa_rank), and every node >= 2 writes its base into the
 * rows of the reads whose bits are set on its out-edges (msa_place_node_full).
 * The consensus row places cons_base[i] at the column of cons_node_ids[i].
 *
 * Two stages, parameterised by (lane, n_lanes), so that the matrix buffer can
 * be sized exactly between them:
 *   - abamd_flat_msa_rank_cols: lane-parallel in-degrees, the rank walk on
 *     lane 0, lane-parallel columns; yields msa_len = rank[SINK] - 1;
 *   - abamd_flat_msa_place: lane-parallel over nodes, then over consensus
 *     positions, into a row-major (rows x msa_len) matrix the caller has
 *     filled with the gap code.
 * The device build (gpu_fold.hip :: abamd_msa_rank_kernel and
 * abamd_msa_place_kernel) runs them across one 64-lane wave; the host build
 * (abamd_fold_core.c) runs the very same code with one lane and is proven
 * against abpoa_generate_rc_msa by tests/test_msa_twin.
 *
 * The device multi-consensus stage builds on the same read rows: one consensus
 * row as a stage of its own (abamd_flat_msa_place_cons_row), and the het scan
 * (abamd_flat_het_count, abamd_flat_het_gather) that finds the candidate
 * heterozygous columns the host clustering needs; gpu_fold.hip wraps them in
 * abamd_cons_row_kernel, abamd_het_count_kernel and abamd_het_gather_kernel,
 * and tests/test_multicons_twin proves them with one lane.
 *
 * Unlike abamd_flat_msa_rank (abamd_fold_core.inc, kept for the fold twin),
 * nothing here aborts: every index read from the graph is range-checked,
 * every chain walk and the stack are bounded, and a graph that fails a check
 * yields ABAMD_MSA_BAD_GRAPH. The graph is only read.
 */

#ifndef ABAMD_FC_BARRIER
#define ABAMD_FC_BARRIER() do { } while (0)
#endif

/* Stage 1a — in-degrees, parallel over nodes; also clears rank[]. A chain
 * that leaves the in-edge pool or is longer than it flags the job. */
ABAMD_FC_FN void abamd_flat_msa_in_deg(const flat_graph_t *fg, int *in_deg, int *rank,
                                       int *stage, int lane, int n_lanes) {
    int i;
    for (i = lane; i < fg->node_n; i += n_lanes) {
        int d = 0, e, ok = 1;
        for (e = fg->in_head[i]; e != -1; e = fg->in_next[e]) {
            if ((unsigned)e >= (unsigned)fg->edge_n_in || d >= fg->edge_n_in) { ok = 0; break; }
            ++d;
        }
        in_deg[i] = d;
        rank[i] = -1;
        if (!ok) stage[0] = ABAMD_MSA_BAD_GRAPH;
    }
}

/* Stage 1b — the LIFO rank walk of dfs_set_msa_rank, on one lane. Its pop
 * order is observable (it is the column order), so it stays serial. Bounds:
 * the stack holds at most node_n entries (a node enters once on a sound
 * graph; a push past that is refused), and every loop iteration draws from
 * one step budget that a sound graph cannot exhaust: <= node_n pops,
 * <= edge_n_out edge visits, and each aligned list is walked at most three
 * times (rank assignment, ready check, push), lists summing to aln_n. */
ABAMD_FC_FN int abamd_flat_msa_walk(const flat_graph_t *fg, int *rank, int *in_deg,
                                    int *stack, int *msa_len_out) {
    const int n = fg->node_n;
    unsigned budget = 4u * ((unsigned)n + (unsigned)fg->edge_n_out + (unsigned)fg->aln_n) + 16u;
    int sp = 0, r = 0, cur, e, a;
    *msa_len_out = 0;
    stack[sp++] = 0; /* SRC */
    rank[0] = -1;
    while (sp > 0) {
        if (!budget--) return ABAMD_MSA_BAD_GRAPH;
        cur = stack[--sp]; /* range-checked when pushed */
        if (rank[cur] < 0) {
            rank[cur] = r;
            for (a = fg->aln_head[cur]; a != -1; a = fg->aln_next[a]) {
                int id;
                if ((unsigned)a >= (unsigned)fg->aln_n || !budget--) return ABAMD_MSA_BAD_GRAPH;
                id = fg->aln_id[a];
                if ((unsigned)id >= (unsigned)n) return ABAMD_MSA_BAD_GRAPH;
                rank[id] = r;
            }
            ++r;
        }
        if (cur == 1 /* SINK */) {
            const int len = rank[1] - 1;
            if (len < 1 || len > n - 2) return ABAMD_MSA_BAD_GRAPH;
            *msa_len_out = len;
            return ABAMD_MSA_OK;
        }
        for (e = fg->out_head[cur]; e != -1; e = fg->out_next[e]) {
            int out, ready = 1;
            if ((unsigned)e >= (unsigned)fg->edge_n_out || !budget--) return ABAMD_MSA_BAD_GRAPH;
            out = fg->out_to[e];
            if ((unsigned)out >= (unsigned)n) return ABAMD_MSA_BAD_GRAPH;
            if (--in_deg[out] != 0) continue;
            for (a = fg->aln_head[out]; a != -1; a = fg->aln_next[a]) {
                int id;
                if ((unsigned)a >= (unsigned)fg->aln_n || !budget--) return ABAMD_MSA_BAD_GRAPH;
                id = fg->aln_id[a];
                if ((unsigned)id >= (unsigned)n) return ABAMD_MSA_BAD_GRAPH;
                if (in_deg[id] != 0) { ready = 0; break; }
            }
            if (!ready) continue;
            if (sp >= n) return ABAMD_MSA_BAD_GRAPH;
            stack[sp++] = out;
            rank[out] = -1;
            for (a = fg->aln_head[out]; a != -1; a = fg->aln_next[a]) {
                int id;
                if ((unsigned)a >= (unsigned)fg->aln_n || !budget-- || sp >= n) return ABAMD_MSA_BAD_GRAPH;
                id = fg->aln_id[a];
                if ((unsigned)id >= (unsigned)n) return ABAMD_MSA_BAD_GRAPH;
                stack[sp++] = id;
                rank[id] = -1;
            }
        }
    }
    return ABAMD_MSA_BAD_GRAPH; /* stack drained before SINK: not a connected DAG */
}

/* Stage 1c — columns, parallel over nodes >= 2: max rank over the node and
 * its aligned group, minus one (group_msa_rank). A node the walk never
 * reached, or a broken aligned list, gets column -1, which the place stage
 * reports if any read passes through it. */
ABAMD_FC_FN void abamd_flat_msa_cols(const flat_graph_t *fg, const int *rank, int *col,
                                     int lane, int n_lanes) {
    int i;
    for (i = 2 + lane; i < fg->node_n; i += n_lanes) {
        int r = rank[i], a, steps = 0, ok = 1;
        for (a = fg->aln_head[i]; a != -1; a = fg->aln_next[a]) {
            int id;
            if ((unsigned)a >= (unsigned)fg->aln_n || ++steps > fg->aln_n) { ok = 0; break; }
            id = fg->aln_id[a];
            if ((unsigned)id >= (unsigned)fg->node_n) { ok = 0; break; }
            if (rank[id] > r) r = rank[id];
        }
        col[i] = (ok && r >= 1) ? r - 1 : -1;
    }
}

/* Stage 1. Every lane of the group calls this with the same arguments and
 * its own lane; all lanes return the same status and see the same
 * *msa_len_out. rank/col/in_deg/stack hold node_n ints each, stage 2 ints
 * shared by the group. */
ABAMD_FC_FN int abamd_flat_msa_rank_cols(const flat_graph_t *fg, int *rank, int *col,
                                         int *in_deg, int *stack, int *stage,
                                         int *msa_len_out, int lane, int n_lanes) {
    int status;
    *msa_len_out = 0;
    if (fg->node_n <= 2 || fg->edge_n_in < 0 || fg->edge_n_out < 0 || fg->aln_n < 0)
        return ABAMD_MSA_BAD_GRAPH;
    if (lane == 0) { stage[0] = ABAMD_MSA_OK; stage[1] = 0; }
    ABAMD_FC_BARRIER();
    abamd_flat_msa_in_deg(fg, in_deg, rank, stage, lane, n_lanes);
    ABAMD_FC_BARRIER();
    status = stage[0];
    ABAMD_FC_BARRIER();
    if (status != ABAMD_MSA_OK) return status;
    if (lane == 0) {
        int len = 0;
        stage[0] = abamd_flat_msa_walk(fg, rank, in_deg, stack, &len);
        stage[1] = len;
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    if (status != ABAMD_MSA_OK) return status;
    abamd_flat_msa_cols(fg, rank, col, lane, n_lanes);
    *msa_len_out = stage[1];
    return ABAMD_MSA_OK;
}

/* One consensus row, parallel over its positions: cons_base[i] goes to the
 * column of cons_id[i] in `row` (msa_len bytes, pre-filled with the gap
 * code). An id outside [2, node_n) or a column outside the row sets stage[0]
 * instead of storing. The caller owns stage[0]'s initial value and the
 * barriers around it. */
ABAMD_FC_FN void abamd_flat_msa_cons_row(int node_n, const int *col, int msa_len, uint8_t *row,
                                         const int *cons_id, const uint8_t *cons_base,
                                         int cons_len, int *stage, int lane, int n_lanes) {
    int i;
    for (i = lane; i < cons_len; i += n_lanes) {
        const int id = cons_id[i];
        int c;
        if (id < 2 || id >= node_n) { stage[0] = ABAMD_MSA_BAD_GRAPH; continue; }
        c = col[id];
        if ((unsigned)c >= (unsigned)msa_len) { stage[0] = ABAMD_MSA_BAD_GRAPH; continue; }
        row[c] = cons_base[i];
    }
}

/* The same as a stage of its own (the multi-consensus path places cluster
 * c's row once that cluster's consensus exists). All lanes return the same
 * status. stage: 2 ints shared by the group. */
ABAMD_FC_FN int abamd_flat_msa_place_cons_row(int node_n, const int *col, int msa_len,
                                              uint8_t *row, const int *cons_id,
                                              const uint8_t *cons_base, int cons_len,
                                              int *stage, int lane, int n_lanes) {
    int status;
    if (lane == 0) stage[0] = ABAMD_MSA_OK;
    ABAMD_FC_BARRIER();
    if (node_n <= 2 || msa_len <= 0 || cons_len < 0 || cons_len > node_n) {
        if (lane == 0) stage[0] = ABAMD_MSA_BAD_GRAPH;
    } else {
        abamd_flat_msa_cons_row(node_n, col, msa_len, row, cons_id, cons_base, cons_len,
                                stage, lane, n_lanes);
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    return status;
}

/* Stage 2 — placement into msa[rows x msa_len] (row-major, pre-filled with
 * the gap code), rows = n_seq read rows plus one consensus row when
 * cons_len >= 0 (pass cons_len < 0 for no consensus row).
 *
 * Parallel over nodes >= 2 with plain stores and no ordering between lanes:
 * ranks strictly increase along every edge and an aligned group shares one
 * rank, so a read's path touches each column at most once; and a read leaves
 * a node through exactly one out-edge, so its bit is set on one edge of the
 * node. Hence no two (node, read) pairs address the same byte. The consensus
 * row is a path too, written parallel over its positions.
 *
 * Nothing is stored out of bounds: a read id >= n_seq, a column outside
 * [0, msa_len), a chain that leaves its pool or a consensus id outside
 * [2, node_n) flags the job instead. All lanes return the same status. */
ABAMD_FC_FN int abamd_flat_msa_place(const flat_graph_t *fg, const int *col, int n_seq,
                                     int msa_len, uint8_t *msa, const int *cons_id,
                                     const uint8_t *cons_base, int cons_len,
                                     int *stage, int lane, int n_lanes) {
    int i, status;
    if (lane == 0) stage[0] = ABAMD_MSA_OK;
    ABAMD_FC_BARRIER();
    if (fg->node_n <= 2 || fg->rid_n <= 0 || n_seq <= 0 || msa_len <= 0 ||
        fg->edge_n_out < 0 || cons_len > fg->node_n) {
        if (lane == 0) stage[0] = ABAMD_MSA_BAD_GRAPH;
    } else {
        for (i = 2 + lane; i < fg->node_n; i += n_lanes) {
            const int c = col[i];
            const uint8_t b = fg->base[i];
            int e, w, steps = 0, ok = 1;
            for (e = fg->out_head[i]; e != -1 && ok; e = fg->out_next[e]) {
                if ((unsigned)e >= (unsigned)fg->edge_n_out || ++steps > fg->edge_n_out) { ok = 0; break; }
                for (w = 0; w < fg->rid_n; ++w) {
                    uint64_t bits = fg->rid_pool[(size_t)e * fg->rid_n + w];
                    while (bits) {
                        const int r = (w << 6) + __builtin_ctzll(bits);
                        bits &= bits - 1;
                        if (r >= n_seq || (unsigned)c >= (unsigned)msa_len) { ok = 0; break; }
                        msa[(size_t)r * msa_len + c] = b;
                    }
                    if (!ok) break;
                }
            }
            if (!ok) stage[0] = ABAMD_MSA_BAD_GRAPH;
        }
        abamd_flat_msa_cons_row(fg->node_n, col, msa_len, msa + (size_t)n_seq * msa_len,
                                cons_id, cons_base, cons_len, stage, lane, n_lanes);
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    return status;
}

/* ------------------------------------------------------------------ */
/* Het scan: the candidate heterozygous columns of the read rows.      */
/* ------------------------------------------------------------------ */

/* Launch 1 — which columns collect_cand_het_pos (abamd_cons.c) would look
 * at: a column is a candidate when at least two of the m + 1 symbols (gap
 * code = m) have min_het <= depth <= min_hom over the n_seq rows. The host
 * derives the two bounds (abamd_het_depth_bounds), so this is integer work
 * only. The multi-consensus stage downloads just these columns; every other
 * column leaves the host clustering before it touches any state.
 *
 * Columns are taken n_lanes at a time, lane l counting column base + l, so a
 * row's byte loads are adjacent across the group; with m <= ABAMD_HET_MAX_M
 * the counters are six scalars. The candidates' column indices go to cand[]
 * in ascending order: per chunk each lane publishes its flag in stage[2 +
 * lane], sums the flags of the lanes before it (its slot) and of all lanes
 * (the running base every lane keeps). A symbol above m, or a candidate past
 * cand_cap, flags the job; nothing is stored out of bounds.
 * stage: ABAMD_HET_STAGE ints shared by the group (n_lanes <= 64). All lanes
 * return the same status and see the same *n_cand_out. */
#define ABAMD_HET_IN(d) ((d) >= min_het && (d) <= min_hom)
ABAMD_FC_FN int abamd_flat_het_count(const uint8_t *msa, int n_seq, int msa_len, int m,
                                     int min_het, int min_hom, int *cand, int cand_cap,
                                     int *stage, int *n_cand_out, int lane, int n_lanes) {
    int base, total = 0, status;
    *n_cand_out = 0;
    if (lane == 0) stage[0] = ABAMD_MSA_OK;
    ABAMD_FC_BARRIER();
    if (n_seq <= 0 || msa_len <= 0 || m < 1 || m > ABAMD_HET_MAX_M || cand_cap < 0 ||
        n_lanes > ABAMD_HET_STAGE - 2) {
        if (lane == 0) stage[0] = ABAMD_MSA_BAD_GRAPH;
    } else {
        for (base = 0; base < msa_len; base += n_lanes) {
            const int c = base + lane;
            int flag = 0, before = 0, all = 0, l;
            if (c < msa_len) {
                int d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, r, ok = 1;
                for (r = 0; r < n_seq; ++r) {
                    const int b = msa[(size_t)r * msa_len + c];
                    d0 += b == 0; d1 += b == 1; d2 += b == 2;
                    d3 += b == 3; d4 += b == 4; d5 += b == 5;
                    if (b > m) ok = 0;
                }
                if (!ok) stage[0] = ABAMD_MSA_BAD_GRAPH;
                /* a counter above m stays 0 on a sound matrix, below min_het >= 2 */
                flag = ok && ABAMD_HET_IN(d0) + ABAMD_HET_IN(d1) + ABAMD_HET_IN(d2) +
                             ABAMD_HET_IN(d3) + ABAMD_HET_IN(d4) + ABAMD_HET_IN(d5) >= 2;
            }
            stage[2 + lane] = flag;
            ABAMD_FC_BARRIER();
            for (l = 0; l < n_lanes; ++l) {
                const int f = stage[2 + l];
                all += f;
                if (l < lane) before += f;
            }
            if (flag) {
                const int k = total + before;
                if (k >= cand_cap) stage[0] = ABAMD_MSA_BAD_GRAPH;
                else cand[k] = c;
            }
            total += all;
            ABAMD_FC_BARRIER(); /* the next chunk rewrites the flags */
        }
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    if (status == ABAMD_MSA_OK) *n_cand_out = total < cand_cap ? total : cand_cap;
    return status;
}
#undef ABAMD_HET_IN

/* Launch 2 — the candidate columns as a row-major n_seq x n_cand matrix,
 * parallel over candidates (a row's stores are adjacent across the group).
 * n_cand is the count launch 1 reported, checked by the host against
 * msa_len; a column index outside the matrix flags the job instead of being
 * read. stage: 2 ints. All lanes return the same status. */
ABAMD_FC_FN int abamd_flat_het_gather(const uint8_t *msa, int n_seq, int msa_len,
                                      const int *cand, int n_cand, uint8_t *out,
                                      int *stage, int lane, int n_lanes) {
    int k, status;
    if (lane == 0) stage[0] = ABAMD_MSA_OK;
    ABAMD_FC_BARRIER();
    if (n_seq <= 0 || msa_len <= 0 || n_cand < 0 || n_cand > msa_len) {
        if (lane == 0) stage[0] = ABAMD_MSA_BAD_GRAPH;
    } else {
        for (k = lane; k < n_cand; k += n_lanes) {
            const int c = cand[k];
            int r;
            if ((unsigned)c >= (unsigned)msa_len) { stage[0] = ABAMD_MSA_BAD_GRAPH; continue; }
            for (r = 0; r < n_seq; ++r)
                out[(size_t)r * n_cand + k] = msa[(size_t)r * msa_len + c];
        }
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    return status;
}

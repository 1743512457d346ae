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
        for (i = lane; i < cons_len; i += n_lanes) {
            const int id = cons_id[i];
            int c;
            if (id < 2 || id >= fg->node_n) { stage[0] = ABAMD_MSA_BAD_GRAPH; continue; }
            c = col[id];
            if ((unsigned)c >= (unsigned)msa_len) { stage[0] = ABAMD_MSA_BAD_GRAPH; continue; }
            msa[(size_t)n_seq * msa_len + c] = cons_base[i];
        }
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    return status;
}

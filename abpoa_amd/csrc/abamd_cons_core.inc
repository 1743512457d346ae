/* abamd_cons_core.inc — shared host/device body for the single-cluster
 * heaviest-bundle consensus over the FLAT graph layout: the device-resident
 * batch driver emits each set's consensus right after its last fold instead
 * of downloading the graph for a host consensus pass.
 *
 * Mirrors heaviest_bundling() for n_clu == 1 (abamd_cons.c; reference
 * abpoa_output.c:478-548 + :376-392): reverse BFS from SINK choosing each
 * node's max-weight out-edge — ties prefer the later-scanned edge when its
 * downstream score is >=, and SRC prefers strictly-higher weight with score
 * as secondary — then the SRC->SINK walk emits ids/bases/coverage.
 * The choice values are pure functions of final successor scores, so any
 * valid reverse-topological visit order gives identical output.
 *
 * Two formulations live here:
 *   - abamd_flat_hb_consensus: the queue-based restatement (out-degree
 *     countdown + reverse BFS), kept as the second witness of the twin tests;
 *   - abamd_flat_cons_phased: the production body. It reuses the topological
 *     order the fold already left in index_to_node_id/node_id_to_index (valid
 *     for rows 0..n2i[SINK]) and runs in four phases parameterised by
 *     (lane, n_lanes): a parallel edge scan, a serial reverse sweep over rows
 *     staged ABAMD_CONS_CHUNK at a time, a bounded serial path walk and a
 *     parallel gather. The device build (gpu_fold.hip::abamd_cons_kernel)
 *     runs it across one 64-lane wave with the staging area in LDS; the host
 *     build runs the very same code with one lane.
 *
 * Included by abamd_fold_core.c (host twin; proven against
 * abpoa_generate_consensus by tests/test_fold_twin and tests/test_cons_twin)
 * and gpu_fold.hip (device build). Phred is NOT computed here on the phased
 * path: it is a pure function of (coverage, n_seq), so the host derives it
 * from the downloaded coverage with cons_phred_score (abamd_cons.c), which
 * also keeps the reference's n_cov > n_seq fatal check. flat_cons_phred below
 * serves the host-only queue-based witness.
 */

#ifndef ABAMD_FC_BARRIER
#define ABAMD_FC_BARRIER() do { } while (0)
#endif

#ifndef ABAMD_CONS_PHASED_ONLY /* host-only witness; the device build skips it */
ABAMD_FC_FN static int flat_cons_phred(int n_cov, int n_seq) {
    double x = 13.8 * (1.25 * n_cov / n_seq - 0.25);
    double p = 1 - 1.0 / (1.0 + pow(2.718281828459045, -1 * x));
    return 33 + (int)(-10 * log10(p) + 0.499);
}

/* returns cons_len; scratch = 2*node_n ints (out-degree + queue);
 * score/max_out = node_n ints; cons_* sized node_n */
ABAMD_FC_FN int abamd_flat_hb_consensus(const flat_graph_t *fg, int n_seq,
                                        int *scratch, int *score, int *max_out,
                                        int *cons_id, uint8_t *cons_base,
                                        int *cons_cov, int *cons_phred) {
    const int n = fg->node_n;
    int *deg = scratch, *q = scratch + n;
    int i, e, cur, qh = 0, qt = 0;
    for (i = 0; i < n; ++i) {
        int d = 0;
        for (e = fg->out_head[i]; e != -1; e = fg->out_next[e]) ++d;
        deg[i] = d;
    }
    q[qt++] = 1; /* SINK */
    while (qh < qt) {
        cur = q[qh++];
        if (cur == 1 /* SINK */) {
            max_out[cur] = -1;
            score[cur] = 0;
        } else if (cur == 0 /* SRC */) {
            int max_id = -1, path_score = -1, path_max_w = -1;
            for (e = fg->out_head[cur]; e != -1; e = fg->out_next[e]) {
                int out_id = fg->out_to[e], w = fg->out_w[e];
                if (w > path_max_w || (w == path_max_w && score[out_id] > path_score)) {
                    max_id = out_id; path_score = score[out_id]; path_max_w = w;
                }
            }
            max_out[cur] = max_id;
            break;
        } else {
            int max_id = -1, max_w = INT32_MIN;
            for (e = fg->out_head[cur]; e != -1; e = fg->out_next[e]) {
                int out_id = fg->out_to[e], w = fg->out_w[e];
                if (max_w < w) { max_w = w; max_id = out_id; }
                else if (max_w == w && score[max_id] <= score[out_id]) max_id = out_id;
            }
            score[cur] = max_w + score[max_id];
            max_out[cur] = max_id;
        }
        for (e = fg->in_head[cur]; e != -1; e = fg->in_next[e]) {
            int in_id = fg->in_to[e];
            if (--deg[in_id] == 0) q[qt++] = in_id;
        }
    }
    int j = 0;
    cur = max_out[0 /* SRC */];
    while (cur != 1 /* SINK */) {
        cons_id[j] = cur;
        cons_base[j] = fg->base[cur];
        cons_cov[j] = fg->n_read[cur];
        cons_phred[j] = flat_cons_phred(fg->n_read[cur], n_seq);
        ++j;
        cur = max_out[cur];
    }
    return j;
}
#endif /* ABAMD_CONS_PHASED_ONLY */

/* ------------------------------------------------------------------ */
/* Phased consensus over the fold's topological order (row space).     */
/* ------------------------------------------------------------------ */

/* Phase 1 — edge scan, parallel over rows. Per row r (node i2n[r]) walk the
 * out-chain once and write IN ROW ORDER the maximum out-edge weight and the
 * successor ROW of the last-scanned edge attaining it. Encoding of best[r]:
 *   >= 0  the single max-weight successor row (untied inner node);
 *   <= -2 ~row: more than one edge attains the maximum, or the node is SRC
 *         (own rule) — phase 2 re-scans the chain with the exact rules;
 *   -1    no usable choice: SINK, or a chain that is not a forward edge list
 *         of this order (index out of its pool, successor row not in
 *         (r, sink_row], chain longer than the pool). Only a corrupt graph
 *         produces the latter; the path walk reports it.
 * Every successor row is checked to be > r, so rows on any path strictly
 * increase and all later loops are bounded by construction.
 * (abamd_flat_cons_edge_scan_clu below is the same scan with cluster-filtered
 * weights; keep the two in step.) */
ABAMD_FC_FN void abamd_flat_cons_edge_scan(const flat_graph_t *fg, const int *i2n,
                                           const int *n2i, int sink_row,
                                           int *max_w, int *best, int lane, int n_lanes) {
    int r;
    for (r = lane; r <= sink_row; r += n_lanes) {
        const int id = i2n[r];
        int w_max = INT32_MIN, b = -1, n_max = 0, ok = 1, steps = 0, e;
        if ((unsigned)id >= (unsigned)fg->node_n || id == 1 /* SINK */) ok = 0;
        else
            for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
                int to, row, w;
                if ((unsigned)e >= (unsigned)fg->edge_n_out || ++steps > fg->edge_n_out) { ok = 0; break; }
                to = fg->out_to[e];
                if ((unsigned)to >= (unsigned)fg->node_n) { ok = 0; break; }
                row = n2i[to];
                if (row <= r || row > sink_row) { ok = 0; break; }
                w = fg->out_w[e];
                if (w > w_max) { w_max = w; b = row; n_max = 1; }
                else if (w == w_max) { b = row; ++n_max; }
            }
        if (!ok || b < 0) { max_w[r] = 0; best[r] = -1; }
        else {
            max_w[r] = w_max;
            best[r] = (n_max > 1 || id == 0 /* SRC */) ? ~b : b;
        }
    }
}

/* score of a successor row: the current chunk's scores live in the staging
 * window, finished chunks in the global row-space array */
ABAMD_FC_FN static int flat_cons_score_at(const int *score, const int *win, int win_base, int row) {
    const unsigned d = (unsigned)(row - win_base);
    return d < (unsigned)ABAMD_CONS_CHUNK ? win[d] : score[row];
}

/* Phase 2, one staged chunk — serial over rows base+hi .. base (one lane).
 * st_w/st_b hold phase 1's results for the chunk; on return win[] holds the
 * chunk's scores and st_b[] the FINAL choices (successor row, or -1).
 * The tied/SRC re-scan is heaviest_bundling's decision logic verbatim, in
 * row space (chains were validated by phase 1, the graph is read-only).
 * abamd_flat_cons_sweep_chunk_clu below restates both rules with
 * cluster-filtered weights: a change to either rule belongs in both. */
ABAMD_FC_FN void abamd_flat_cons_sweep_chunk(const flat_graph_t *fg, const int *i2n,
                                             const int *n2i, int base, int sink_row,
                                             const int *score, const int *st_w,
                                             int *st_b, int *win) {
    int l = sink_row - base, e;
    if (l > ABAMD_CONS_CHUNK - 1) l = ABAMD_CONS_CHUNK - 1;
    for (; l >= 0; --l) {
        const int b = st_b[l];
        if (b >= 0) {
            win[l] = st_w[l] + flat_cons_score_at(score, win, base, b);
        } else if (b == -1) {
            win[l] = 0; /* SINK (score 0) or an unusable row */
        } else {
            const int id = i2n[base + l];
            if (id == 0 /* SRC */) {
                int max_row = -1, path_score = -1, path_max_w = -1;
                for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
                    const int row = n2i[fg->out_to[e]], w = fg->out_w[e];
                    const int sc = flat_cons_score_at(score, win, base, row);
                    if (w > path_max_w || (w == path_max_w && sc > path_score)) {
                        max_row = row; path_score = sc; path_max_w = w;
                    }
                }
                st_b[l] = max_row;
                win[l] = 0;
            } else {
                int max_row = -1, mw = INT32_MIN;
                for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
                    const int row = n2i[fg->out_to[e]], w = fg->out_w[e];
                    if (mw < w) { mw = w; max_row = row; }
                    else if (mw == w && flat_cons_score_at(score, win, base, max_row) <=
                                        flat_cons_score_at(score, win, base, row)) max_row = row;
                }
                st_b[l] = max_row;
                win[l] = mw + flat_cons_score_at(score, win, base, max_row);
            }
        }
    }
}

/* Phase 2 — reverse sweep over rows sink_row .. 0, ABAMD_CONS_CHUNK rows at
 * a time: all lanes stage phase 1's results (coalesced), lane 0 runs the
 * chunk, all lanes write scores and final choices back (coalesced). stage =
 * 3*ABAMD_CONS_CHUNK ints (LDS on the device). */
ABAMD_FC_FN void abamd_flat_cons_sweep(const flat_graph_t *fg, const int *i2n, const int *n2i,
                                       int sink_row, const int *max_w, int *best, int *score,
                                       int *stage, int lane, int n_lanes) {
    int *st_w = stage, *st_b = stage + ABAMD_CONS_CHUNK, *win = stage + 2 * ABAMD_CONS_CHUNK;
    int base, l;
    for (base = (sink_row / ABAMD_CONS_CHUNK) * ABAMD_CONS_CHUNK; base >= 0; base -= ABAMD_CONS_CHUNK) {
        for (l = lane; l < ABAMD_CONS_CHUNK; l += n_lanes)
            if (base + l <= sink_row) { st_w[l] = max_w[base + l]; st_b[l] = best[base + l]; }
        ABAMD_FC_BARRIER();
        if (lane == 0)
            abamd_flat_cons_sweep_chunk(fg, i2n, n2i, base, sink_row, score, st_w, st_b, win);
        ABAMD_FC_BARRIER();
        for (l = lane; l < ABAMD_CONS_CHUNK; l += n_lanes)
            if (base + l <= sink_row) { score[base + l] = win[l]; best[base + l] = st_b[l]; }
        ABAMD_FC_BARRIER();
    }
}

/* Phase 3 — path walk from SRC's choice to SINK through the final best[]
 * (one lane). Bounded by sink_row + 1 steps; a choice of -1 or a walk past
 * the bound is a corrupt graph. Returns the status; *len_out = rows walked. */
ABAMD_FC_FN int abamd_flat_cons_walk(const int *best, int sink_row, int *path, int *len_out) {
    int j = 0, cur = best[0];
    *len_out = 0;
    while (cur != sink_row) {
        if (cur < 0 || cur > sink_row || j > sink_row) return ABAMD_CONS_BAD_GRAPH;
        path[j++] = cur;
        cur = best[cur];
    }
    *len_out = j;
    return ABAMD_CONS_OK;
}

/* Phase 4 — gather, parallel over path positions. cons_id may alias path
 * (each position is read then written by the same lane). */
ABAMD_FC_FN void abamd_flat_cons_gather(const flat_graph_t *fg, const int *i2n, const int *path,
                                        int cons_len, int *cons_id, uint8_t *cons_base,
                                        int *cons_cov, int lane, int n_lanes) {
    int j;
    for (j = lane; j < cons_len; j += n_lanes) {
        const int id = i2n[path[j]];
        cons_id[j] = id;
        cons_base[j] = fg->base[id];
        cons_cov[j] = fg->n_read[id];
    }
}

/* The four phases in order. Every lane of the group calls this with the
 * same arguments and its own lane; all lanes return the same status and see
 * the same *cons_len_out. Workspaces max_w/best/score/path hold n2i[SINK]+1
 * ints each, cons_* up to n2i[SINK] entries; stage = 3*ABAMD_CONS_CHUNK
 * ints shared by the group. The graph, i2n and n2i are only read. */
ABAMD_FC_FN int abamd_flat_cons_phased(const flat_graph_t *fg, const int *i2n, const int *n2i,
                                       int *max_w, int *best, int *score, int *path,
                                       int *cons_id, uint8_t *cons_base, int *cons_cov,
                                       int *stage, int *cons_len_out, int lane, int n_lanes) {
    int sink_row, status, len;
    *cons_len_out = 0;
    if (fg->node_n <= 2) return ABAMD_CONS_BAD_GRAPH;
    sink_row = n2i[1 /* SINK */];
    if (sink_row <= 0 || sink_row >= fg->node_n || n2i[0 /* SRC */] != 0 ||
        i2n[0] != 0 || i2n[sink_row] != 1)
        return ABAMD_CONS_BAD_GRAPH;
    abamd_flat_cons_edge_scan(fg, i2n, n2i, sink_row, max_w, best, lane, n_lanes);
    ABAMD_FC_BARRIER();
    abamd_flat_cons_sweep(fg, i2n, n2i, sink_row, max_w, best, score, stage, lane, n_lanes);
    if (lane == 0) {
        int wl = 0;
        stage[0] = abamd_flat_cons_walk(best, sink_row, path, &wl);
        stage[1] = wl;
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    len = stage[1];
    if (status != ABAMD_CONS_OK) return status;
    abamd_flat_cons_gather(fg, i2n, path, len, cons_id, cons_base, cons_cov, lane, n_lanes);
    *cons_len_out = len;
    return ABAMD_CONS_OK;
}

/* ------------------------------------------------------------------ */
/* Cluster-filtered variant (multi-consensus, n_clu >= 2).             */
/* ------------------------------------------------------------------ */

/* One heaviest-bundle pass of heaviest_bundling() for cluster `mask`
 * (rid_n words): the four phases above with two differences. An edge's
 * weight is the number of the cluster's reads on it (inclu_edge_weight
 * without use_qv), popcount(rid_pool[e] & mask) summed over the words, in
 * the phase-1 scan and in both re-scan rules; zero-weight ties are the
 * normal case at nodes only another cluster's reads visit, so far more rows
 * take the re-scan than with stored weights. And the gathered coverage is the
 * sum of those counts over the node's out-edges: the reference's
 * abpoa_node_cov, whose in-side term is always 0 (node_cov_clu,
 * abamd_cons.c). The text is kept apart from the single-cluster functions so
 * that their code, and abamd_cons_kernel's registers, stay as they are. */
ABAMD_FC_FN static int flat_cons_w_clu(const flat_graph_t *fg, const uint64_t *mask, int e) {
    int w, n = 0;
    for (w = 0; w < fg->rid_n; ++w)
        n += __builtin_popcountll(fg->rid_pool[(size_t)e * fg->rid_n + w] & mask[w]);
    return n;
}

/* Phase 1, as abamd_flat_cons_edge_scan (same encoding of best[], same chain
 * checks) */
ABAMD_FC_FN void abamd_flat_cons_edge_scan_clu(const flat_graph_t *fg, const uint64_t *mask,
                                               const int *i2n, const int *n2i, int sink_row,
                                               int *max_w, int *best, int lane, int n_lanes) {
    int r;
    for (r = lane; r <= sink_row; r += n_lanes) {
        const int id = i2n[r];
        int w_max = INT32_MIN, b = -1, n_max = 0, ok = 1, steps = 0, e;
        if ((unsigned)id >= (unsigned)fg->node_n || id == 1 /* SINK */) ok = 0;
        else
            for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
                int to, row, w;
                if ((unsigned)e >= (unsigned)fg->edge_n_out || ++steps > fg->edge_n_out) { ok = 0; break; }
                to = fg->out_to[e];
                if ((unsigned)to >= (unsigned)fg->node_n) { ok = 0; break; }
                row = n2i[to];
                if (row <= r || row > sink_row) { ok = 0; break; }
                w = flat_cons_w_clu(fg, mask, e);
                if (w > w_max) { w_max = w; b = row; n_max = 1; }
                else if (w == w_max) { b = row; ++n_max; }
            }
        if (!ok || b < 0) { max_w[r] = 0; best[r] = -1; }
        else {
            max_w[r] = w_max;
            best[r] = (n_max > 1 || id == 0 /* SRC */) ? ~b : b;
        }
    }
}

/* Phase 2, one staged chunk, as abamd_flat_cons_sweep_chunk */
ABAMD_FC_FN void abamd_flat_cons_sweep_chunk_clu(const flat_graph_t *fg, const uint64_t *mask,
                                                 const int *i2n, const int *n2i, int base,
                                                 int sink_row, const int *score, const int *st_w,
                                                 int *st_b, int *win) {
    int l = sink_row - base, e;
    if (l > ABAMD_CONS_CHUNK - 1) l = ABAMD_CONS_CHUNK - 1;
    for (; l >= 0; --l) {
        const int b = st_b[l];
        if (b >= 0) {
            win[l] = st_w[l] + flat_cons_score_at(score, win, base, b);
        } else if (b == -1) {
            win[l] = 0; /* SINK (score 0) or an unusable row */
        } else {
            const int id = i2n[base + l];
            if (id == 0 /* SRC */) {
                int max_row = -1, path_score = -1, path_max_w = -1;
                for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
                    const int row = n2i[fg->out_to[e]], w = flat_cons_w_clu(fg, mask, e);
                    const int sc = flat_cons_score_at(score, win, base, row);
                    if (w > path_max_w || (w == path_max_w && sc > path_score)) {
                        max_row = row; path_score = sc; path_max_w = w;
                    }
                }
                st_b[l] = max_row;
                win[l] = 0;
            } else {
                int max_row = -1, mw = INT32_MIN;
                for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
                    const int row = n2i[fg->out_to[e]], w = flat_cons_w_clu(fg, mask, e);
                    if (mw < w) { mw = w; max_row = row; }
                    else if (mw == w && flat_cons_score_at(score, win, base, max_row) <=
                                        flat_cons_score_at(score, win, base, row)) max_row = row;
                }
                st_b[l] = max_row;
                win[l] = mw + flat_cons_score_at(score, win, base, max_row);
            }
        }
    }
}

/* Phase 2, as abamd_flat_cons_sweep */
ABAMD_FC_FN void abamd_flat_cons_sweep_clu(const flat_graph_t *fg, const uint64_t *mask,
                                           const int *i2n, const int *n2i, int sink_row,
                                           const int *max_w, int *best, int *score,
                                           int *stage, int lane, int n_lanes) {
    int *st_w = stage, *st_b = stage + ABAMD_CONS_CHUNK, *win = stage + 2 * ABAMD_CONS_CHUNK;
    int base, l;
    for (base = (sink_row / ABAMD_CONS_CHUNK) * ABAMD_CONS_CHUNK; base >= 0; base -= ABAMD_CONS_CHUNK) {
        for (l = lane; l < ABAMD_CONS_CHUNK; l += n_lanes)
            if (base + l <= sink_row) { st_w[l] = max_w[base + l]; st_b[l] = best[base + l]; }
        ABAMD_FC_BARRIER();
        if (lane == 0)
            abamd_flat_cons_sweep_chunk_clu(fg, mask, i2n, n2i, base, sink_row, score, st_w, st_b, win);
        ABAMD_FC_BARRIER();
        for (l = lane; l < ABAMD_CONS_CHUNK; l += n_lanes)
            if (base + l <= sink_row) { score[base + l] = win[l]; best[base + l] = st_b[l]; }
        ABAMD_FC_BARRIER();
    }
}

/* Phase 4: ids and bases as abamd_flat_cons_gather; coverage = the cluster's
 * reads over the node's out-edges. Every path row passed phase 1's chain
 * checks (a row that failed them has best = -1, which ends the walk), and the
 * walk here is bounded again all the same. */
ABAMD_FC_FN void abamd_flat_cons_gather_clu(const flat_graph_t *fg, const uint64_t *mask,
                                            const int *i2n, const int *path, int cons_len,
                                            int *cons_id, uint8_t *cons_base, int *cons_cov,
                                            int lane, int n_lanes) {
    int j;
    for (j = lane; j < cons_len; j += n_lanes) {
        const int id = i2n[path[j]];
        int cov = 0, steps = 0, e;
        for (e = fg->out_head[id]; e != -1; e = fg->out_next[e]) {
            if ((unsigned)e >= (unsigned)fg->edge_n_out || ++steps > fg->edge_n_out) break;
            cov += flat_cons_w_clu(fg, mask, e);
        }
        cons_id[j] = id;
        cons_base[j] = fg->base[id];
        cons_cov[j] = cov;
    }
}

/* The four phases for one cluster; arguments as abamd_flat_cons_phased plus
 * the cluster's mask of fg->rid_n words (only read). */
ABAMD_FC_FN int abamd_flat_cons_phased_clu(const flat_graph_t *fg, const uint64_t *mask,
                                           const int *i2n, const int *n2i,
                                           int *max_w, int *best, int *score, int *path,
                                           int *cons_id, uint8_t *cons_base, int *cons_cov,
                                           int *stage, int *cons_len_out, int lane, int n_lanes) {
    int sink_row, status, len;
    *cons_len_out = 0;
    if (fg->node_n <= 2 || fg->rid_n <= 0 || fg->edge_n_out < 0) return ABAMD_CONS_BAD_GRAPH;
    sink_row = n2i[1 /* SINK */];
    if (sink_row <= 0 || sink_row >= fg->node_n || n2i[0 /* SRC */] != 0 ||
        i2n[0] != 0 || i2n[sink_row] != 1)
        return ABAMD_CONS_BAD_GRAPH;
    abamd_flat_cons_edge_scan_clu(fg, mask, i2n, n2i, sink_row, max_w, best, lane, n_lanes);
    ABAMD_FC_BARRIER();
    abamd_flat_cons_sweep_clu(fg, mask, i2n, n2i, sink_row, max_w, best, score, stage, lane, n_lanes);
    if (lane == 0) {
        int wl = 0;
        stage[0] = abamd_flat_cons_walk(best, sink_row, path, &wl);
        stage[1] = wl;
    }
    ABAMD_FC_BARRIER();
    status = stage[0];
    len = stage[1];
    if (status != ABAMD_CONS_OK) return status;
    abamd_flat_cons_gather_clu(fg, mask, i2n, path, len, cons_id, cons_base, cons_cov, lane, n_lanes);
    *cons_len_out = len;
    return ABAMD_CONS_OK;
}

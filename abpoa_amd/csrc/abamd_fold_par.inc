/* abamd_fold_par.inc — deterministic lane-parallel form of the graph
 * mutation walk (abamd_flat_apply_alignment, abamd_fold_core.inc), shared by
 * the host build (abamd_fold_core.c; tests/test_fold_par_twin.py runs it with
 * one lane and with 64 emulated lanes against the serial walk) and the device
 * build (gpu_fold.hip :: abamd_fold_round_kernel, one 64-lane wave per set).
 *
 * Why it can be parallel. What the serial walk leaves behind is fixed by
 * three things only: the order in which pool slots are handed out (node ids,
 * in/out edge ids, aligned-pool ids), the position at which an entry is
 * appended to a per-node chain, and the values stored. A CIGAR describes one
 * SRC->SINK path, so each graph node is visited at most once: every in-chain,
 * out-chain and aligned group that the walk reads or appends to belongs to
 * exactly one op. The slot orders are then exclusive prefix sums over the
 * CIGAR, and everything else is independent per op / per path edge.
 *
 * Phases (all lanes call each phase, a barrier separates them; lane l owns
 * the contiguous block l of the ops, and of the path edges):
 *   0  query bases consumed per op                      -> per-lane sums
 *   1  classify (match / aligned member / new node / insertion / deletion),
 *      count new nodes and aligned-pool entries, claim the op's node and its
 *      aligned group in the owner array                 -> per-lane sums
 *   2  verify the claims; new node ids by prefix sum; path node and inherited
 *      n_span_read of every query position              -> path[], nsp[]
 *   3  per path edge: search the in-chain of `to` and the out-chain of `from`
 *      exactly as flat_add_edge does                    -> e_in[], e_out[]
 *   4  all lanes take the same keep-or-fall-back decision; then the writes:
 *      edge weights, new edges at the chain tails, read-id bits, n_read, node
 *      bases, n_span_read, the qpos map, aligned-pair entries
 *   5  the four counters
 * Phases 0-3 write scratch only. They do not rely on the one-visit property,
 * they check it: every op claims its node and the members of its aligned
 * group (owner[id] = op index) and re-reads the claims after a barrier, so
 * two ops that share a node or a group cannot both see their own index; every
 * id is range-checked, every chain walk is bounded by its pool count. Any
 * violation, or a pool that would overflow, makes every lane skip phase 4:
 * the graph is untouched and the caller runs the serial walk instead
 * (abamd_flat_apply_par returns 0).
 *
 * Cross-lane prefix sums go through flat_par_excl over a per-lane array in
 * scratch, so a host loop over lanes per phase emulates a wave exactly.
 *
 * Scratch (flat_par_ws_t): six int arrays of `cap` entries and `part` of
 * ABAMD_PAR_PARTS * n_lanes entries. Needs n_cigar <= cap and seq_l + 1 <=
 * cap; otherwise the serial walk runs. */

#ifndef ABAMD_FC_BARRIER
#define ABAMD_FC_BARRIER() do { } while (0)
#endif
/* the per-lane arrays are read in short serial loops; the device build keeps
 * them rolled (64 loads unrolled side by side cost 64 registers per loop) */
#ifndef ABAMD_FC_ROLLED
#define ABAMD_FC_ROLLED
#endif

enum { FLAT_PAR_SERIAL = 0, FLAT_PAR_EMPTY = 1, FLAT_PAR_CHAIN = 2, FLAT_PAR_WALK = 3 };

/* exclusive prefix of lane's entry in a per-lane array, and the total */
ABAMD_FC_FN static int flat_par_excl(const int *p, int lane, int n_lanes, int *total) {
    int l, s = 0, ex = 0;
    ABAMD_FC_ROLLED
    for (l = 0; l < n_lanes; ++l) {
        if (l == lane) ex = s;
        s += p[l];
    }
    *total = s;
    return ex;
}

/* lane's contiguous block [*lo, *hi) of n items */
ABAMD_FC_FN static void flat_par_block(int n, int lane, int n_lanes, int *lo, int *hi) {
    const int b = (n + n_lanes - 1) / n_lanes;
    long l0 = (long)lane * b;
    if (l0 > n) l0 = n;
    *lo = (int)l0;
    *hi = (int)(l0 + b > n ? n : l0 + b);
}

/* query bases an op consumes; an insertion longer than the read is a
 * violation (flagged by phase 0) and consumes nothing in every phase */
ABAMD_FC_FN static int flat_par_consumed(abpoa_cigar_t c, int seq_l, int *bad) {
    const int op = (int)(c & 0xf);
    if (op == ABPOA_CMATCH) return 1;
    if (op == ABPOA_CINS || op == ABPOA_CSOFT_CLIP || op == ABPOA_CHARD_CLIP) {
        const int len = (int)((c >> 4) & 0x3fffffff);
        if (len > seq_l) { *bad = 1; return 0; }
        return len;
    }
    return 0;
}

ABAMD_FC_FN static int flat_par_node_ok(const flat_par_t *cx, int id) {
    return (unsigned)id < (unsigned)cx->node_n0 && id != cx->beg && id != cx->end;
}

ABAMD_FC_FN void abamd_flat_par_init(flat_par_t *cx, flat_graph_t *fg, int beg_node_id,
                                     int end_node_id, const uint8_t *seq, const int *weight,
                                     int seq_l, int *qpos_to_node_id, int n_cigar,
                                     const abpoa_cigar_t *cig, int read_id, int add_read_id,
                                     int inc_both_ends, const flat_par_ws_t *ws, int n_lanes) {
    cx->fg = fg; cx->beg = beg_node_id; cx->end = end_node_id;
    cx->seq = seq; cx->weight = weight; cx->seq_l = seq_l; cx->qpos = qpos_to_node_id;
    cx->n_cigar = n_cigar; cx->cig = cig;
    cx->read_id = read_id; cx->add_read_id = add_read_id; cx->inc_both_ends = inc_both_ends;
    cx->node_n0 = fg->node_n; cx->ein0 = fg->edge_n_in; cx->eout0 = fg->edge_n_out;
    cx->aln0 = fg->aln_n;
    cx->ws = *ws;
    cx->ok = 0;
    if (fg->node_n == 2) { /* first read: plain chain */
        const long need = (long)seq_l + 1;
        cx->mode = (seq_l >= 1 && 2 + (long)seq_l <= fg->node_cap &&
                    fg->edge_n_in + need <= fg->edge_cap && fg->edge_n_out + need <= fg->edge_cap)
                   ? FLAT_PAR_CHAIN : FLAT_PAR_SERIAL;
    } else if (n_cigar == 0) {
        cx->mode = FLAT_PAR_EMPTY;
    } else {
        cx->mode = (n_lanes >= 1 && ws->part_cap >= ABAMD_PAR_PARTS * n_lanes &&
                    n_cigar <= ws->cap && seq_l >= 1 && (long)seq_l + 1 <= ws->cap &&
                    (unsigned)beg_node_id < (unsigned)fg->node_n &&
                    (unsigned)end_node_id < (unsigned)fg->node_n && beg_node_id != end_node_id)
                   ? FLAT_PAR_WALK : FLAT_PAR_SERIAL;
    }
}

/* phase 0: consumed query bases, per-lane sum */
ABAMD_FC_FN static void flat_par_p0(flat_par_t *cx, int lane, int n_lanes) {
    int lo, hi, i, bad = 0, c = 0;
    flat_par_block(cx->n_cigar, lane, n_lanes, &lo, &hi);
    for (i = lo; i < hi; ++i) {
        c += flat_par_consumed(cx->cig[i], cx->seq_l, &bad);
        if (c > cx->seq_l) { bad = 1; c = 0; break; }
    }
    cx->ws.part[FLAT_PAR_BAD * n_lanes + lane] = bad;
    cx->ws.part[FLAT_PAR_C * n_lanes + lane] = bad ? 0 : c;
}

/* phase 1: classification, counts, ownership claims. A lane that phase 0
 * flagged does nothing more (its block's query offsets are unknown). */
ABAMD_FC_FN static void flat_par_p1(flat_par_t *cx, int lane, int n_lanes) {
    const flat_graph_t *fg = cx->fg;
    int *part = cx->ws.part;
    int lo, hi, i, q_tot, nn = 0, na = 0, last = -1;
    int bad = part[FLAT_PAR_BAD * n_lanes + lane];
    int q = flat_par_excl(part + FLAT_PAR_C * n_lanes, lane, n_lanes, &q_tot);
    if (q_tot > cx->seq_l) bad = 1; /* more query than the read has: every lane sees it */
    flat_par_block(cx->n_cigar, lane, n_lanes, &lo, &hi);
    for (i = lo; i < hi && !bad; ++i) {
        const abpoa_cigar_t c = cx->cig[i];
        const int op = (int)(c & 0xf);
        if (op == ABPOA_CMATCH) {
            const int nid = (int)((c >> 34) & 0x3fffffff);
            int res = cx->beg; /* any valid id: a flagged op is never applied */
            if (!flat_par_node_ok(cx, nid) || q >= cx->seq_l) bad = 1;
            else {
                const uint8_t b = cx->seq[q];
                int a, g = 0, found = -1, steps = 0;
                cx->ws.owner[nid] = i;
                for (a = fg->aln_head[nid]; a != -1; a = fg->aln_next[a]) {
                    int m;
                    if ((unsigned)a >= (unsigned)cx->aln0 || ++steps > cx->aln0) { bad = 1; break; }
                    m = fg->aln_id[a];
                    if (!flat_par_node_ok(cx, m)) { bad = 1; break; }
                    cx->ws.owner[m] = i;
                    if (found < 0 && fg->base[m] == b) found = m;
                    ++g;
                }
                if (!bad) {
                    if (fg->base[nid] == b) res = nid;
                    else if (found >= 0) res = found;
                    else { res = -1; nn += 1; na += 2 * g + 2; }
                }
            }
            cx->ws.opres[i] = res;
            if (res >= 0) last = res;
            q += 1;
        } else {
            int dummy = 0;
            const int len = flat_par_consumed(c, cx->seq_l, &dummy);
            nn += len;
            q += len;
        }
    }
    part[FLAT_PAR_BAD * n_lanes + lane] = bad;
    part[FLAT_PAR_NN * n_lanes + lane] = bad ? 0 : nn;
    part[FLAT_PAR_NA * n_lanes + lane] = bad ? 0 : na;
    part[FLAT_PAR_LAST * n_lanes + lane] = bad ? -1 : last;
}

/* phase 2: verify the claims, then path node and inherited n_span_read per
 * query position (scratch only; new ids are not dereferenced here) */
ABAMD_FC_FN static void flat_par_p2(flat_par_t *cx, int lane, int n_lanes) {
    const flat_graph_t *fg = cx->fg;
    int *part = cx->ws.part;
    int lo, hi, i, l, q_tot, nn_tot;
    int bad = part[FLAT_PAR_BAD * n_lanes + lane];
    int q = flat_par_excl(part + FLAT_PAR_C * n_lanes, lane, n_lanes, &q_tot);
    int new_id = cx->node_n0 + flat_par_excl(part + FLAT_PAR_NN * n_lanes, lane, n_lanes, &nn_tot);
    int anchor = cx->beg, anchor_val = 0, have_val = 0;
    if (bad) return;
    ABAMD_FC_ROLLED
    for (l = lane - 1; l >= 0; --l)
        if (part[FLAT_PAR_LAST * n_lanes + l] >= 0) { anchor = part[FLAT_PAR_LAST * n_lanes + l]; break; }
    flat_par_block(cx->n_cigar, lane, n_lanes, &lo, &hi);
    for (i = lo; i < hi && !bad; ++i) {
        const abpoa_cigar_t c = cx->cig[i];
        const int op = (int)(c & 0xf);
        if (op == ABPOA_CMATCH) {
            const int nid = (int)((c >> 34) & 0x3fffffff);
            const int res = cx->ws.opres[i];
            int a, steps = 0;
            if (cx->ws.owner[nid] != i) bad = 1;
            for (a = fg->aln_head[nid]; a != -1 && !bad; a = fg->aln_next[a]) {
                if ((unsigned)a >= (unsigned)cx->aln0 || ++steps > cx->aln0) { bad = 1; break; }
                if (cx->ws.owner[fg->aln_id[a]] != i) bad = 1;
            }
            if (bad) break;
            if (res >= 0) {
                cx->ws.path[q] = res;
                anchor = res; have_val = 0;
            } else {
                if (!have_val) { anchor_val = fg->n_span_read[anchor]; have_val = 1; }
                cx->ws.path[q] = new_id++;
                cx->ws.nsp[q] = anchor_val;
            }
            q += 1;
        } else {
            int dummy = 0, t;
            const int len = flat_par_consumed(c, cx->seq_l, &dummy);
            if (len > 0 && !have_val) { anchor_val = fg->n_span_read[anchor]; have_val = 1; }
            for (t = 0; t < len; ++t) {
                cx->ws.path[q + t] = new_id++;
                cx->ws.nsp[q + t] = anchor_val;
            }
            q += len;
        }
    }
    part[FLAT_PAR_BAD * n_lanes + lane] = bad;
}

/* phase 3: per path edge k (from path[k-1] or beg, to path[k] or end), the
 * existing-edge search of flat_add_edge with check_edge = 1 - last_new (and 0
 * for a new target): both ends must be old nodes */
ABAMD_FC_FN static void flat_par_p3(flat_par_t *cx, int lane, int n_lanes) {
    const flat_graph_t *fg = cx->fg;
    int *part = cx->ws.part;
    int lo, hi, k, l, q_tot, ne = 0, bad = 0;
    (void)flat_par_excl(part + FLAT_PAR_C * n_lanes, lane, n_lanes, &q_tot);
    ABAMD_FC_ROLLED
    for (l = 0; l < n_lanes; ++l) bad |= part[FLAT_PAR_BAD * n_lanes + l];
    if (bad) { part[FLAT_PAR_NE * n_lanes + lane] = 0; return; } /* path[] is incomplete */
    flat_par_block(q_tot + 1, lane, n_lanes, &lo, &hi);
    for (k = lo; k < hi; ++k) {
        const int from = k ? cx->ws.path[k - 1] : cx->beg;
        const int to = k < q_tot ? cx->ws.path[k] : cx->end;
        int e, e_in = -1, e_out = -1, steps;
        if (from < cx->node_n0 && to < cx->node_n0) {
            for (e = fg->in_head[to], steps = 0; e != -1; e = fg->in_next[e]) {
                if ((unsigned)e >= (unsigned)cx->ein0 || ++steps > cx->ein0) { bad = 1; break; }
                if (fg->in_to[e] == from) { e_in = e; break; }
            }
            for (e = fg->out_head[from], steps = 0; e != -1 && !bad; e = fg->out_next[e]) {
                if ((unsigned)e >= (unsigned)cx->eout0 || ++steps > cx->eout0) { bad = 1; break; }
                if (fg->out_to[e] == to) { e_out = e; break; }
            }
        }
        cx->ws.e_in[k] = e_in;
        cx->ws.e_out[k] = e_out;
        if (e_out < 0) ++ne;
    }
    part[FLAT_PAR_BAD * n_lanes + lane] = bad;
    part[FLAT_PAR_NE * n_lanes + lane] = ne;
}

/* append pool entry a to the tail of node id's aligned chain */
ABAMD_FC_FN static void flat_par_aln_append(flat_graph_t *fg, int id, int a, int bound) {
    int t = fg->aln_head[id], steps = 0;
    if ((unsigned)t >= (unsigned)fg->aln_cap) { fg->aln_head[id] = a; return; } /* -1: empty */
    while (fg->aln_next[t] != -1 && (unsigned)fg->aln_next[t] < (unsigned)fg->aln_cap &&
           ++steps <= bound) t = fg->aln_next[t];
    fg->aln_next[t] = a;
}

/* phase 4: the decision, then every write of the serial walk */
ABAMD_FC_FN static void flat_par_p4(flat_par_t *cx, int lane, int n_lanes) {
    flat_graph_t *fg = cx->fg;
    int *part = cx->ws.part;
    int lo, hi, i, k, l, q_tot, nn_tot, na_tot, ne_tot, bad = 0;
    int nn_off, na_off, ne_off;
    ABAMD_FC_ROLLED
    for (l = 0; l < n_lanes; ++l) bad |= part[FLAT_PAR_BAD * n_lanes + l];
    (void)flat_par_excl(part + FLAT_PAR_C * n_lanes, lane, n_lanes, &q_tot);
    nn_off = flat_par_excl(part + FLAT_PAR_NN * n_lanes, lane, n_lanes, &nn_tot);
    na_off = flat_par_excl(part + FLAT_PAR_NA * n_lanes, lane, n_lanes, &na_tot);
    ne_off = flat_par_excl(part + FLAT_PAR_NE * n_lanes, lane, n_lanes, &ne_tot);
    if ((long)cx->node_n0 + nn_tot > fg->node_cap || (long)cx->aln0 + na_tot > fg->aln_cap ||
        (long)cx->ein0 + ne_tot > fg->edge_cap || (long)cx->eout0 + ne_tot > fg->edge_cap)
        bad = 1;
    cx->ok = !bad;
    if (bad) return;
    cx->nn_tot = nn_tot; cx->na_tot = na_tot; cx->ne_tot = ne_tot;

    /* edges, nodes, qpos */
    flat_par_block(q_tot + 1, lane, n_lanes, &lo, &hi);
    for (k = lo; k < hi; ++k) {
        const int from = k ? cx->ws.path[k - 1] : cx->beg;
        const int to = k < q_tot ? cx->ws.path[k] : cx->end;
        const int w = k < q_tot ? cx->weight[k] : cx->weight[cx->seq_l - 1];
        const int add = k < q_tot ? ((k > 0 || cx->inc_both_ends) ? 1 : 0) : 1;
        const int add_rid = k < q_tot ? (cx->add_read_id & add) : cx->add_read_id;
        const int e_in = cx->ws.e_in[k];
        int e_out = cx->ws.e_out[k];
        if (e_in >= 0) fg->in_w[e_in] += w;
        if (e_out >= 0) fg->out_w[e_out] += w;
        else {
            int e = cx->ein0 + ne_off, t;
            fg->in_to[e] = from; fg->in_w[e] = w; fg->in_next[e] = -1;
            t = fg->in_tail[to];
            if (t == -1) fg->in_head[to] = e;
            else fg->in_next[t] = e;
            fg->in_tail[to] = e;
            e = cx->eout0 + ne_off;
            fg->out_to[e] = to; fg->out_w[e] = w; fg->out_next[e] = -1;
            t = fg->out_tail[from];
            if (t == -1) fg->out_head[from] = e;
            else fg->out_next[t] = e;
            fg->out_tail[from] = e;
            e_out = e;
            ++ne_off;
        }
        if (add_rid && fg->rid_n > 0)
            fg->rid_pool[(size_t)e_out * fg->rid_n + (cx->read_id >> 6)] |= 1ull << (cx->read_id & 0x3f);
        if (add) fg->n_read[from] += 1;
        if (k < q_tot) {
            if (to >= cx->node_n0) {
                fg->base[to] = cx->seq[k];
                fg->n_span_read[to] = cx->ws.nsp[k];
            }
            if (cx->qpos) cx->qpos[k] = to;
        }
    }

    /* aligned-pair entries, in flat_add_aligned_pair's allocation order: per
     * group member m (chain order of the op's node) entry A+2j = new_id at
     * m's tail and A+2j+1 = m in new_id's chain; then A+2g = new_id at the
     * node's tail and A+2g+1 = the node, the end of new_id's chain */
    flat_par_block(cx->n_cigar, lane, n_lanes, &lo, &hi);
    {
        int new_id = cx->node_n0 + nn_off, a_next = cx->aln0 + na_off;
        for (i = lo; i < hi; ++i) {
            const abpoa_cigar_t c = cx->cig[i];
            const int op = (int)(c & 0xf);
            if (op == ABPOA_CMATCH) {
                if (cx->ws.opres[i] < 0) {
                    const int nid = (int)((c >> 34) & 0x3fffffff);
                    int a, A = a_next, tail = -1, steps = 0;
                    for (a = fg->aln_head[nid]; a != -1 && ++steps <= cx->aln0; a = fg->aln_next[a]) {
                        const int m = fg->aln_id[a];
                        fg->aln_id[A] = new_id; fg->aln_next[A] = -1;
                        flat_par_aln_append(fg, m, A, cx->aln0);
                        fg->aln_id[A + 1] = m; fg->aln_next[A + 1] = A + 3;
                        A += 2;
                        tail = a;
                    }
                    fg->aln_id[A] = new_id; fg->aln_next[A] = -1;
                    if (tail == -1) fg->aln_head[nid] = A;
                    else fg->aln_next[tail] = A;
                    fg->aln_id[A + 1] = nid; fg->aln_next[A + 1] = -1;
                    fg->aln_head[new_id] = a_next + 1;
                    a_next = A + 2;
                    ++new_id;
                }
            } else {
                int dummy = 0;
                new_id += flat_par_consumed(c, cx->seq_l, &dummy);
            }
        }
    }
}

/* first read: nodes 2..seq_l+1 in a chain SRC -> ... -> SINK, edge k gets the
 * k-th slot of both pools (flat_add_edge with check_edge = 0 throughout) */
ABAMD_FC_FN static void flat_par_chain(flat_par_t *cx, int lane, int n_lanes) {
    flat_graph_t *fg = cx->fg;
    const int span0 = fg->n_span_read[0 /* SRC */];
    int k;
    for (k = lane; k <= cx->seq_l; k += n_lanes) {
        const int from = k ? cx->node_n0 + k - 1 : 0 /* SRC */;
        const int to = k < cx->seq_l ? cx->node_n0 + k : 1 /* SINK */;
        const int w = cx->weight[k < cx->seq_l ? k : cx->seq_l - 1];
        int e = cx->ein0 + k, t;
        fg->in_to[e] = from; fg->in_w[e] = w; fg->in_next[e] = -1;
        t = fg->in_tail[to];
        if (t == -1) fg->in_head[to] = e;
        else fg->in_next[t] = e;
        fg->in_tail[to] = e;
        e = cx->eout0 + k;
        fg->out_to[e] = to; fg->out_w[e] = w; fg->out_next[e] = -1;
        t = fg->out_tail[from];
        if (t == -1) fg->out_head[from] = e;
        else fg->out_next[t] = e;
        fg->out_tail[from] = e;
        if (cx->add_read_id && fg->rid_n > 0)
            fg->rid_pool[(size_t)e * fg->rid_n + (cx->read_id >> 6)] |= 1ull << (cx->read_id & 0x3f);
        fg->n_read[from] += 1;
        if (k < cx->seq_l) {
            fg->base[to] = cx->seq[k];
            fg->n_span_read[to] = span0;
            if (cx->qpos) cx->qpos[k] = to;
        }
    }
    cx->ok = 1;
    cx->nn_tot = cx->seq_l; cx->na_tot = 0; cx->ne_tot = cx->seq_l + 1;
}

/* one phase for one lane; phases run 0 .. ABAMD_PAR_PHASES-1 with a barrier
 * after each (a host emulation of n lanes loops the lanes inside a phase) */
ABAMD_FC_FN void abamd_flat_par_phase(flat_par_t *cx, int phase, int lane, int n_lanes) {
    if (cx->mode == FLAT_PAR_SERIAL) return;
    if (cx->mode == FLAT_PAR_EMPTY) { cx->ok = 1; return; }
    if (cx->mode == FLAT_PAR_CHAIN) {
        if (phase == 4) flat_par_chain(cx, lane, n_lanes);
    } else {
        if (phase == 0) flat_par_p0(cx, lane, n_lanes);
        else if (phase == 1) flat_par_p1(cx, lane, n_lanes);
        else if (phase == 2) flat_par_p2(cx, lane, n_lanes);
        else if (phase == 3) flat_par_p3(cx, lane, n_lanes);
        else if (phase == 4) flat_par_p4(cx, lane, n_lanes);
    }
    if (phase == 5 && cx->ok) { /* every lane stores the same totals */
        flat_graph_t *fg = cx->fg;
        fg->node_n = cx->node_n0 + cx->nn_tot;
        fg->edge_n_in = cx->ein0 + cx->ne_tot;
        fg->edge_n_out = cx->eout0 + cx->ne_tot;
        fg->aln_n = cx->aln0 + cx->na_tot;
    }
}

/* The whole walk. Every lane of the group calls this with the same arguments
 * and its own lane; all lanes return the same value: 1 = applied (or an empty
 * CIGAR on an existing graph, which applies nothing), 0 = graph untouched,
 * the caller runs abamd_flat_apply_alignment. */
ABAMD_FC_FN int abamd_flat_apply_par(flat_graph_t *fg, int beg_node_id, int end_node_id,
                                     const uint8_t *seq, const int *weight, int seq_l,
                                     int *qpos_to_node_id, int n_cigar, const abpoa_cigar_t *cig,
                                     int read_id, int add_read_id, int inc_both_ends,
                                     const flat_par_ws_t *ws, int lane, int n_lanes) {
    flat_par_t cx;
    int phase;
    abamd_flat_par_init(&cx, fg, beg_node_id, end_node_id, seq, weight, seq_l, qpos_to_node_id,
                        n_cigar, cig, read_id, add_read_id, inc_both_ends, ws, n_lanes);
    if (cx.mode == FLAT_PAR_SERIAL) return 0;
    if (cx.mode == FLAT_PAR_EMPTY) return 1;
    for (phase = 0; phase < ABAMD_PAR_PHASES; ++phase) {
        abamd_flat_par_phase(&cx, phase, lane, n_lanes);
        if (phase < ABAMD_PAR_PHASES - 1) ABAMD_FC_BARRIER();
    }
    return cx.ok;
}

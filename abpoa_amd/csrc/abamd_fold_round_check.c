/* Per-round check of the production fold kernel (abamd_fold_round_kernel,
 * gpu_fold.hip) against the serial flat-graph twin — see
 * abamd_fold_round_check.h. The twin's pass order is the one
 * tests/test_fold_twin.py pins to the pointer graph:
 *   apply_alignment, topo_index, sort_adjacency, remain, update_n_span,
 *   build_rows.
 * Everything the kernel's own passes write is compared, after every fold:
 * counters, every pool and chain array with heads and tails, read-id
 * bitsets, the topological order and its inverse over the prefix up to SINK,
 * max_remain over that prefix, and the seven DP-row CSR arrays. */
#include <stdlib.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"
#include "abamd_fold_core.h"
#include "abamd_fold_round_check.h"

typedef struct {
    int init, next_read;
    flat_graph_t g;
    int *i2n, *n2i, *rem, *scr, *w;
    uint8_t *row_base;
    int *row_node_id, *pre_off, *out_off, *row_remain, *pre_idx, *out_idx;
    int node_cap, edge_cap, aln_cap;   /* the DEVICE's caps at the previous call */
    int last_rows;
} frc_set_t;

struct abamd_frc_t {
    int m, use_read_ids, n_sets;
    const int *n_seqs;
    const int *const *seq_lens;
    const uint8_t *const *const *seqs;
    frc_set_t *sets;
    int failed;
    long folds, noop, walks[3];
    int max_in_deg, max_out_deg, max_n_rows, min_n_rows, caps_grew;
};

abamd_frc_t *abamd_frc_new(const abpoa_para_t *abpt, int n_sets, const int *n_seqs,
                           const int *const *seq_lens, const uint8_t *const *const *seqs) {
    abamd_frc_t *c = (abamd_frc_t*)abamd_calloc(1, sizeof(*c));
    c->m = abpt->m; c->use_read_ids = abpt->use_read_ids ? 1 : 0;
    c->n_sets = n_sets; c->n_seqs = n_seqs; c->seq_lens = seq_lens; c->seqs = seqs;
    c->sets = (frc_set_t*)abamd_calloc(n_sets > 0 ? n_sets : 1, sizeof(frc_set_t));
    c->min_n_rows = -1;
    return c;
}

static void set_init(abamd_frc_t *c, int s) {
    frc_set_t *t = &c->sets[s];
    int64_t L = 0;
    int i, max_len = 1, n = c->n_seqs[s];
    for (i = 0; i < n; ++i) {
        L += c->seq_lens[s][i];
        if (c->seq_lens[s][i] > max_len) max_len = c->seq_lens[s][i];
    }
    /* a read adds at most len nodes, len + 1 edges per direction and, per new
     * node, 2 (m - 1) aligned-pool entries */
    const int nc = (int)L + 2 + 8, ec = (int)L + n + 8, ac = (int)(2 * (int64_t)c->m * L) + 1024;
    abamd_flat_init(&t->g, nc, ec, ac, c->use_read_ids ? 1 + ((n - 1) >> 6) : 0);
    t->i2n = (int*)abamd_calloc(nc, sizeof(int));
    t->n2i = (int*)abamd_calloc(nc, sizeof(int));
    t->rem = (int*)abamd_calloc(nc, sizeof(int));
    t->scr = (int*)abamd_calloc(2 * (size_t)nc, sizeof(int));
    t->w = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    for (i = 0; i < max_len; ++i) t->w[i] = 1;
    t->row_base = (uint8_t*)abamd_calloc(nc, 1);
    t->row_node_id = (int*)abamd_calloc(nc, sizeof(int));
    t->pre_off = (int*)abamd_calloc((size_t)nc + 1, sizeof(int));
    t->out_off = (int*)abamd_calloc((size_t)nc + 1, sizeof(int));
    t->row_remain = (int*)abamd_calloc(nc, sizeof(int));
    t->pre_idx = (int*)abamd_calloc(ec, sizeof(int));
    t->out_idx = (int*)abamd_calloc(ec, sizeof(int));
    t->init = 1;
}

void abamd_frc_free(abamd_frc_t *c) {
    int s;
    if (!c) return;
    for (s = 0; s < c->n_sets; ++s) {
        frc_set_t *t = &c->sets[s];
        if (!t->init) continue;
        abamd_flat_free(&t->g);
        free(t->i2n); free(t->n2i); free(t->rem); free(t->scr); free(t->w);
        free(t->row_base); free(t->row_node_id); free(t->pre_off); free(t->out_off);
        free(t->row_remain); free(t->pre_idx); free(t->out_idx);
    }
    free(c->sets);
    free(c);
}

int abamd_frc_failed(const abamd_frc_t *c) { return c->failed; }

static int bad(abamd_frc_t *c, const abpoa_amd_fold_probe_t *p, FILE *err, const char *field,
               long index, long long dev, long long twin) {
    fprintf(err, "fold-check MISMATCH set %d read %d field %s index %ld: device %lld twin %lld\n",
            p->set_idx, p->read_idx, field, index, dev, twin);
    fflush(err);
    c->failed = 1;
    return 1;
}

#define CMP_VAL(field, dev, twin) do { \
    if ((long long)(dev) != (long long)(twin)) return bad(c, p, err, field, -1, (dev), (twin)); } while (0)
#define CMP_ARR(field, dptr, tptr, count) do { long _k, _n = (long)(count); \
    for (_k = 0; _k < _n; ++_k) if ((dptr)[_k] != (tptr)[_k]) \
        return bad(c, p, err, field, _k, (long long)(dptr)[_k], (long long)(tptr)[_k]); } while (0)

int abamd_frc_check(abamd_frc_t *c, const abpoa_amd_fold_probe_t *p, FILE *err) {
    if (c->failed) return 1;
    if (p->set_idx < 0 || p->set_idx >= c->n_sets) return bad(c, p, err, "set_idx", -1, p->set_idx, c->n_sets);
    const int s = p->set_idx;
    frc_set_t *t = &c->sets[s];
    if (!t->init) set_init(c, s);
    flat_graph_t *g = &t->g;
    CMP_VAL("read_idx", p->read_idx, t->next_read);
    if (p->read_idx >= c->n_seqs[s]) return bad(c, p, err, "read_idx", -1, p->read_idx, c->n_seqs[s]);
    t->next_read += 1;
    CMP_VAL("rid_n", p->rid_n, g->rid_n);
    if (t->node_cap && (p->node_cap > t->node_cap || p->edge_cap > t->edge_cap || p->aln_cap > t->aln_cap))
        c->caps_grew = 1;
    t->node_cap = p->node_cap; t->edge_cap = p->edge_cap; t->aln_cap = p->aln_cap;

    if (p->status == ABPOA_AMD_FOLD_PROBE_NOOP) {
        /* the reference folds nothing for an empty CIGAR on an existing graph:
         * the twin stays, and the counters the kernel reports are its own */
        c->noop += 1;
        CMP_VAL("node_n", p->out.node_n, g->node_n);
        CMP_VAL("edge_n_in", p->out.edge_n_in, g->edge_n_in);
        CMP_VAL("edge_n_out", p->out.edge_n_out, g->edge_n_out);
        CMP_VAL("aln_n", p->out.aln_n, g->aln_n);
        return 0;
    }
    CMP_VAL("status", p->status, ABPOA_AMD_FOLD_PROBE_OK);
    CMP_VAL("walk", p->walk, p->out.walk);
    if (p->walk < 0 || p->walk > 2) return bad(c, p, err, "walk", -1, p->walk, 2);
    if (p->read_idx == 0) CMP_VAL("n_cigar", p->n_cigar, 0);
    /* the kernel's own capacity pre-check, restated: what it wrote fits */
    if (p->out.node_n > p->node_cap) return bad(c, p, err, "node_cap", -1, p->out.node_n, p->node_cap);
    if (p->out.edge_n_in > p->edge_cap || p->out.edge_n_out > p->edge_cap)
        return bad(c, p, err, "edge_cap", -1, p->out.edge_n_out, p->edge_cap);
    if (p->out.aln_n > p->aln_cap) return bad(c, p, err, "aln_cap", -1, p->out.aln_n, p->aln_cap);

    /* ---- advance the twin ---- */
    const int qlen = c->seq_lens[s][p->read_idx];
    abamd_flat_apply_alignment(g, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, c->seqs[s][p->read_idx],
                               t->w, qlen, NULL, p->n_cigar, (const abpoa_cigar_t*)p->cigar,
                               p->read_idx, c->use_read_ids, 1);
    abamd_flat_topo_index(g, t->i2n, t->n2i, t->scr);
    abamd_flat_sort_adjacency(g);
    abamd_flat_remain(g, t->rem, t->scr);
    abamd_flat_update_n_span(g, t->i2n, t->n2i, 1);
    const int n_rows = abamd_flat_build_rows(g, t->i2n, t->n2i, t->rem, p->use_remain,
                                             t->row_base, t->row_node_id, t->pre_off, t->out_off,
                                             t->row_remain, t->pre_idx, t->out_idx);
    const int n_pre = t->pre_off[n_rows], n_out = t->out_off[n_rows];

    /* ---- statistics (from the twin: they describe the input) ---- */
    c->folds += 1;
    c->walks[p->walk] += 1;
    t->last_rows = n_rows;
    if (n_rows > c->max_n_rows) c->max_n_rows = n_rows;
    if (c->min_n_rows < 0 || n_rows < c->min_n_rows) c->min_n_rows = n_rows;
    {
        int r;
        for (r = 0; r < n_rows; ++r) {
            int di = t->pre_off[r + 1] - t->pre_off[r], dq = t->out_off[r + 1] - t->out_off[r];
            if (di > c->max_in_deg) c->max_in_deg = di;
            if (dq > c->max_out_deg) c->max_out_deg = dq;
        }
    }

    /* ---- counters ---- */
    CMP_VAL("node_n", p->out.node_n, g->node_n);
    CMP_VAL("edge_n_in", p->out.edge_n_in, g->edge_n_in);
    CMP_VAL("edge_n_out", p->out.edge_n_out, g->edge_n_out);
    CMP_VAL("aln_n", p->out.aln_n, g->aln_n);
    CMP_VAL("n_rows", p->out.n_rows, n_rows);
    CMP_VAL("n_pre", p->out.n_pre, n_pre);
    CMP_VAL("n_out", p->out.n_out, n_out);

    /* ---- graph ---- */
    const int n = g->node_n;
    CMP_ARR("base", p->base, g->base, n);
    CMP_ARR("n_read", p->n_read, g->n_read, n);
    CMP_ARR("n_span_read", p->n_span_read, g->n_span_read, n);
    CMP_ARR("in_head", p->in_head, g->in_head, n);
    CMP_ARR("in_tail", p->in_tail, g->in_tail, n);
    CMP_ARR("out_head", p->out_head, g->out_head, n);
    CMP_ARR("out_tail", p->out_tail, g->out_tail, n);
    CMP_ARR("aln_head", p->aln_head, g->aln_head, n);
    CMP_ARR("in_to", p->in_to, g->in_to, g->edge_n_in);
    CMP_ARR("in_w", p->in_w, g->in_w, g->edge_n_in);
    CMP_ARR("in_next", p->in_next, g->in_next, g->edge_n_in);
    CMP_ARR("out_to", p->out_to, g->out_to, g->edge_n_out);
    CMP_ARR("out_w", p->out_w, g->out_w, g->edge_n_out);
    CMP_ARR("out_next", p->out_next, g->out_next, g->edge_n_out);
    if (g->rid_n > 0)
        CMP_ARR("rid_pool", p->rid_pool, g->rid_pool, (long)g->edge_n_out * g->rid_n);
    CMP_ARR("aln_id", p->aln_id, g->aln_id, g->aln_n);
    CMP_ARR("aln_next", p->aln_next, g->aln_next, g->aln_n);

    /* ---- topological order over the prefix the DP reads, and remain ---- */
    CMP_ARR("i2n", p->i2n, t->i2n, n_rows);
    {
        int k;
        for (k = 0; k < n_rows; ++k) {
            const int id = t->i2n[k];
            if (p->n2i[id] != t->n2i[id]) return bad(c, p, err, "n2i", id, p->n2i[id], t->n2i[id]);
        }
        if (p->use_remain)
            for (k = 0; k < n_rows; ++k) {
                const int id = t->i2n[k];
                if (p->rem[id] != t->rem[id]) return bad(c, p, err, "rem", id, p->rem[id], t->rem[id]);
            }
    }

    /* ---- DP-row CSR ---- */
    CMP_ARR("row_base", p->row_base, t->row_base, n_rows);
    CMP_ARR("row_node_id", p->row_node_id, t->row_node_id, n_rows);
    CMP_ARR("pre_off", p->pre_off, t->pre_off, n_rows + 1);
    CMP_ARR("out_off", p->out_off, t->out_off, n_rows + 1);
    CMP_ARR("row_remain", p->row_remain, t->row_remain, n_rows);
    if (!p->use_remain) {
        int r;
        for (r = 0; r < n_rows; ++r)
            if (p->row_remain[r] != 0) return bad(c, p, err, "row_remain", r, p->row_remain[r], 0);
    }
    CMP_ARR("pre_idx", p->pre_idx, t->pre_idx, n_pre);
    CMP_ARR("out_idx", p->out_idx, t->out_idx, n_out);
    return 0;
}

void abamd_frc_summary(const abamd_frc_t *c, FILE *f) {
    int s;
    fprintf(f, "[fold-check] folds=%ld noop=%ld parallel=%ld fallback=%ld serial=%ld "
               "max_in_deg=%d max_out_deg=%d max_n_rows=%d min_n_rows=%d caps_grew=%d rows_by_set=",
            c->folds, c->noop, c->walks[1], c->walks[2], c->walks[0],
            c->max_in_deg, c->max_out_deg, c->max_n_rows, c->min_n_rows < 0 ? 0 : c->min_n_rows,
            c->caps_grew);
    for (s = 0; s < c->n_sets; ++s) fprintf(f, "%s%d", s ? "," : "", c->sets[s].last_rows);
    fprintf(f, "\n");
}

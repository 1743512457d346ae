/* Parallel-fold twin test driver: replays every read of a FASTA through the
 * serial flat mutation walk (abamd_flat_apply_alignment) and through the
 * lane-parallel phased walk (abamd_fold_par.inc), the latter twice: with one
 * lane, and with 64 lanes emulated on the host (all lanes run phase k before
 * any lane runs phase k+1, which is what the device barrier gives). The three
 * flat graphs are fed the same oracle CIGARs; after every read the phased
 * graphs must equal the serial one in every field: the four counters, node
 * bases, n_read, n_span_read, chain heads and tails, the edge and aligned
 * pools up to their counts, the read-id words and the qpos->node map.
 *
 * Built against gpu_stub.c so the aligner is the injected oracle
 * (ABPOA_AMD_TEST_ALIGNER_SO). Usage: abpoa_amd_foldpartwin reads.fa [-r1] [-v]
 * -r1 turns read-id tracking on; -v prints one line per read with its op
 * count and insertion lengths. Prints "partwin OK (...)" on success with the
 * number of folds that fell back to the serial walk and whether any read's
 * intermediate state differed between the 1-lane and the 64-lane partition.
 * -g adds a guard self-test after the last read: three corrupted copies of
 * its CIGAR (one node visited twice, a node id beyond the pool, an insertion
 * longer than the read) must each make the phased walk return 0 with the
 * graph left exactly as it was; prints "guards OK". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"
#include "abamd_fold_core.h"

typedef struct abamd_fx_t abamd_fx_t;
abpoa_seq_t *abamd_seq_new(void);
void abamd_seq_destroy(abpoa_seq_t *abs);
abamd_fx_t *abamd_fx_open(const char *fn);
void abamd_fx_close(abamd_fx_t *x);
int abamd_read_seq(abpoa_seq_t *abs, abamd_fx_t *x);

#define EMU_LANES 64

static void die(const char *what, int read_i, int lanes) {
    fprintf(stderr, "PAR TWIN MISMATCH after read %d (%d lanes): %s\n", read_i, lanes, what);
    exit(1);
}

static void ws_init(flat_par_ws_t *ws, int cap, int n_lanes) {
    ws->cap = cap;
    ws->owner = (int*)abamd_malloc((size_t)cap * sizeof(int));
    ws->path = (int*)abamd_malloc((size_t)cap * sizeof(int));
    ws->nsp = (int*)abamd_malloc((size_t)cap * sizeof(int));
    ws->opres = (int*)abamd_malloc((size_t)cap * sizeof(int));
    ws->e_in = (int*)abamd_malloc((size_t)cap * sizeof(int));
    ws->e_out = (int*)abamd_malloc((size_t)cap * sizeof(int));
    ws->part_cap = ABAMD_PAR_PARTS * n_lanes;
    ws->part = (int*)abamd_calloc((size_t)ws->part_cap, sizeof(int));
    /* stale claims must not matter: start from a value that is a valid op index */
    memset(ws->owner, 0, (size_t)cap * sizeof(int));
}

static void ws_free(flat_par_ws_t *ws) {
    free(ws->owner); free(ws->path); free(ws->nsp); free(ws->opres);
    free(ws->e_in); free(ws->e_out); free(ws->part);
}

#define CMP(field, count, T, what) do { \
    if (memcmp(a->field, b->field, (size_t)(count) * sizeof(T))) die(what, read_i, lanes); } while (0)

static void compare(const flat_graph_t *a, const flat_graph_t *b, int read_i, int lanes) {
    if (a->node_n != b->node_n) die("node_n", read_i, lanes);
    if (a->edge_n_in != b->edge_n_in) die("edge_n_in", read_i, lanes);
    if (a->edge_n_out != b->edge_n_out) die("edge_n_out", read_i, lanes);
    if (a->aln_n != b->aln_n) die("aln_n", read_i, lanes);
    CMP(base, a->node_n, uint8_t, "base");
    CMP(n_read, a->node_n, int, "n_read");
    CMP(n_span_read, a->node_n, int, "n_span_read");
    CMP(in_head, a->node_n, int, "in_head");
    CMP(in_tail, a->node_n, int, "in_tail");
    CMP(out_head, a->node_n, int, "out_head");
    CMP(out_tail, a->node_n, int, "out_tail");
    CMP(aln_head, a->node_n, int, "aln_head");
    CMP(in_to, a->edge_n_in, int, "in_to");
    CMP(in_w, a->edge_n_in, int, "in_w");
    CMP(in_next, a->edge_n_in, int, "in_next");
    CMP(out_to, a->edge_n_out, int, "out_to");
    CMP(out_w, a->edge_n_out, int, "out_w");
    CMP(out_next, a->edge_n_out, int, "out_next");
    CMP(aln_id, a->aln_n, int, "aln_id");
    CMP(aln_next, a->aln_n, int, "aln_next");
    if (a->rid_n > 0) CMP(rid_pool, (size_t)a->edge_n_out * a->rid_n, uint64_t, "rid_pool");
}

/* the derived passes every fold runs, in the live order; n_span_read feeds
 * the next read's new nodes */
static void derive(flat_graph_t *fg, int *i2n, int *n2i, int *scr) {
    abamd_flat_topo_index(fg, i2n, n2i, scr);
    abamd_flat_sort_adjacency(fg);
    abamd_flat_update_n_span(fg, i2n, n2i, 1);
}

/* run the phased walk over all lanes of an emulated wave; returns its verdict */
static int emulate(flat_graph_t *fg, const uint8_t *codes, const int *w, int qlen, int *qmap,
                   int n_cigar, const abpoa_cigar_t *cig, int read_id, int add_read_id,
                   const flat_par_ws_t *ws, int n_lanes) {
    flat_par_t cx;
    int phase, lane;
    abamd_flat_par_init(&cx, fg, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w, qlen,
                        qmap, n_cigar, cig, read_id, add_read_id, 1, ws, n_lanes);
    for (phase = 0; phase < ABAMD_PAR_PHASES; ++phase)
        for (lane = 0; lane < n_lanes; ++lane)
            abamd_flat_par_phase(&cx, phase, lane, n_lanes);
    return cx.ok;
}

int main(int argc, char **argv) {
    int a, verbose = 0, guards = 0;
    abpoa_cigar_t *last_cig = NULL;
    int last_n_cigar = 0;
    if (argc < 2) { fprintf(stderr, "usage: %s reads.fa [-r1] [-v]\n", argv[0]); return 2; }
    abpoa_para_t *abpt = abpoa_init_para();
    for (a = 2; a < argc; ++a) {
        if (strcmp(argv[a], "-r1") == 0) abpt->out_msa = 1;
        else if (strcmp(argv[a], "-v") == 0) verbose = 1;
        else if (strcmp(argv[a], "-g") == 0) guards = 1;
    }
    abpoa_post_set_para(abpt);
    abpoa_t *ab = abpoa_init();
    abpoa_reset(ab, abpt, 1024);

    abpoa_seq_t *abs = abamd_seq_new();
    abamd_fx_t *fx = abamd_fx_open(argv[1]);
    int n_seq = abamd_read_seq(abs, fx);
    abamd_fx_close(fx);
    ab->abs->n_seq = n_seq;

    int total_len = 0, max_len = 0, i, j;
    for (i = 0; i < n_seq; ++i) {
        total_len += abs->seq[i].l;
        if (abs->seq[i].l > max_len) max_len = abs->seq[i].l;
    }
    const int rid_n = abpt->use_read_ids ? 1 + ((n_seq - 1) >> 6) : 0;
    const int node_cap = total_len + 2, edge_cap = 4 * total_len + 64, aln_cap = 8 * total_len + 1024;
    const int ws_cap = 2 * total_len + 66; /* >= n_cigar <= qlen + rows, and seq_l + 1 */
    flat_graph_t gs, g1, g64;
    abamd_flat_init(&gs, node_cap, edge_cap, aln_cap, rid_n);
    abamd_flat_init(&g1, node_cap, edge_cap, aln_cap, rid_n);
    abamd_flat_init(&g64, node_cap, edge_cap, aln_cap, rid_n);
    flat_par_ws_t ws1, ws64;
    ws_init(&ws1, ws_cap, 1);
    ws_init(&ws64, ws_cap, EMU_LANES);

    int *w = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    int *qs = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    int *q1 = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    int *q64 = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    int *i2n = (int*)abamd_malloc((size_t)node_cap * sizeof(int));
    int *n2i = (int*)abamd_malloc((size_t)node_cap * sizeof(int));
    int *scr = (int*)abamd_malloc((size_t)2 * node_cap * sizeof(int));
    uint8_t *codes = (uint8_t*)abamd_malloc((size_t)max_len);
    for (i = 0; i < max_len; ++i) w[i] = 1;

    int fallbacks = 0, differs = 0;
    for (i = 0; i < n_seq; ++i) {
        const int qlen = abs->seq[i].l;
        for (j = 0; j < qlen; ++j) codes[j] = (uint8_t)ab_amd_char26_table[(int)abs->seq[i].s[j]];
        const int prev_nodes = gs.node_n, prev_edges = gs.edge_n_out;
        abpoa_res_t res; memset(&res, 0, sizeof(res));
        abpoa_align_sequence_to_graph(ab, abpt, codes, qlen, &res);
        if (res.n_cigar > ws_cap) die("n_cigar beyond the workspace", i, 0);

        abamd_flat_apply_alignment(&gs, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w, qlen,
                                   qs, res.n_cigar, res.graph_cigar, i, abpt->use_read_ids, 1);
        /* one lane */
        if (!abamd_flat_apply_par(&g1, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w, qlen,
                                  q1, res.n_cigar, res.graph_cigar, i, abpt->use_read_ids, 1,
                                  &ws1, 0, 1)) {
            ++fallbacks;
            abamd_flat_apply_alignment(&g1, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w, qlen,
                                       q1, res.n_cigar, res.graph_cigar, i, abpt->use_read_ids, 1);
        }
        /* 64 emulated lanes: lane loop per phase */
        if (!emulate(&g64, codes, w, qlen, q64, res.n_cigar, res.graph_cigar, i,
                     abpt->use_read_ids, &ws64, EMU_LANES)) {
            ++fallbacks;
            abamd_flat_apply_alignment(&g64, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w,
                                       qlen, q64, res.n_cigar, res.graph_cigar, i,
                                       abpt->use_read_ids, 1);
        }
        if (guards && i == n_seq - 1 && res.n_cigar) {
            last_n_cigar = res.n_cigar;
            last_cig = (abpoa_cigar_t*)abamd_malloc((size_t)res.n_cigar * sizeof(abpoa_cigar_t));
            memcpy(last_cig, res.graph_cigar, (size_t)res.n_cigar * sizeof(abpoa_cigar_t));
        }
        /* the partitions really differ: lane 0 of 64 consumed less query than
         * the single lane did */
        if (i > 0 && res.n_cigar > 0 &&
            ws64.part[FLAT_PAR_C * EMU_LANES] != ws1.part[FLAT_PAR_C]) differs = 1;
        if (verbose) {
            int k, max_ins = 0, first_ins = 0, last_ins = 0, qpos = 0;
            for (k = 0; k < res.n_cigar; ++k) {
                int op = (int)(res.graph_cigar[k] & 0xf);
                int len = (int)((res.graph_cigar[k] >> 4) & 0x3fffffff);
                if (op == ABPOA_CMATCH) qpos += 1;
                else if (op == ABPOA_CINS || op == ABPOA_CSOFT_CLIP || op == ABPOA_CHARD_CLIP) {
                    if (len > max_ins) max_ins = len;
                    if (qpos == 0) first_ins = len;
                    if (qpos + len == qlen) last_ins = len;
                    qpos += len;
                }
            }
            printf("read %d n_cigar %d max_ins %d first_ins %d last_ins %d new_nodes %d new_edges %d\n",
                   i, res.n_cigar, max_ins, first_ins, last_ins,
                   gs.node_n - prev_nodes, gs.edge_n_out - prev_edges);
        }
        abpoa_add_graph_alignment(ab, abpt, codes, w, qlen, NULL, res, i, n_seq, 1);
        if (res.n_cigar) free(res.graph_cigar);

        compare(&gs, &g1, i, 1);
        compare(&gs, &g64, i, EMU_LANES);
        for (j = 0; j < qlen; ++j) {
            if (qs[j] != q1[j]) die("qpos_to_node_id", i, 1);
            if (qs[j] != q64[j]) die("qpos_to_node_id", i, EMU_LANES);
        }
        derive(&gs, i2n, n2i, scr);
        derive(&g1, i2n, n2i, scr);
        derive(&g64, i2n, n2i, scr);
    }
    if (fallbacks) { fprintf(stderr, "PAR TWIN: %d folds fell back to the serial walk\n", fallbacks); return 1; }
    if (guards) {
        /* codes/w still hold the last read; the three graphs are equal */
        const int qlen = abs->seq[n_seq - 1].l;
        int m0 = -1, m1 = -1, v, k;
        for (k = 0; k < last_n_cigar; ++k)
            if ((last_cig[k] & 0xf) == ABPOA_CMATCH) { if (m0 < 0) m0 = k; else { m1 = k; break; } }
        if (m1 < 0) die("guard self-test needs two match ops in the last read", n_seq - 1, 0);
        for (v = 0; v < 3; ++v) {
            abpoa_cigar_t *c = (abpoa_cigar_t*)abamd_malloc((size_t)last_n_cigar * sizeof(abpoa_cigar_t));
            const abpoa_cigar_t keep = ((abpoa_cigar_t)1 << 34) - 1;
            memcpy(c, last_cig, (size_t)last_n_cigar * sizeof(abpoa_cigar_t));
            if (v == 0) c[m1] = (c[m1] & keep) | (c[m0] & ~keep);            /* node visited twice */
            else if (v == 1) c[m1] = (c[m1] & keep) | ((abpoa_cigar_t)gs.node_n << 34); /* id beyond the pool */
            else c[m1] = ((abpoa_cigar_t)(qlen + 1) << 4) | ABPOA_CINS;       /* insertion > read */
            if (abamd_flat_apply_par(&g1, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w, qlen,
                                     q1, last_n_cigar, c, n_seq, abpt->use_read_ids, 1, &ws1, 0, 1))
                die("guard did not trip", v, 1);
            if (emulate(&g64, codes, w, qlen, q64, last_n_cigar, c, n_seq, abpt->use_read_ids,
                        &ws64, EMU_LANES))
                die("guard did not trip", v, EMU_LANES);
            compare(&gs, &g1, -1 - v, 1);
            compare(&gs, &g64, -1 - v, EMU_LANES);
            free(c);
        }
        free(last_cig);
        printf("guards OK\n");
    }
    printf("partwin OK (%d reads, %d nodes, %d out-edges, %d aligned entries, fallbacks %d, "
           "partition differs %d)\n", n_seq, gs.node_n, gs.edge_n_out, gs.aln_n, fallbacks, differs);
    ws_free(&ws1); ws_free(&ws64);
    abamd_flat_free(&gs); abamd_flat_free(&g1); abamd_flat_free(&g64);
    free(w); free(qs); free(q1); free(q64); free(i2n); free(n2i); free(scr); free(codes);
    abamd_seq_destroy(abs);
    abpoa_free(ab);
    abpoa_free_para(abpt);
    return 0;
}

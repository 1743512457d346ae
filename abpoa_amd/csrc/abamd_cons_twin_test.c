/* Consensus-twin test driver: replays every read of a FASTA through the
 * pointer-based graph fold (abamd_graph.c) and the flat-array device-layout
 * core (abamd_fold_core.c) and, after EVERY read, runs the phased flat
 * consensus (abamd_cons_core.inc :: abamd_flat_cons_phased — the body of the
 * device consensus kernel, here with one lane) over the flat graph and its
 * index_to_node_id/node_id_to_index, assembles an abpoa_cons_t through
 * abamd_cons_from_path (the device-resident driver's result builder) and
 * compares every field against abpoa_generate_consensus on the live pointer
 * graph: n_cons, n_seq, cons_len, node ids, bases, coverage, phred,
 * clu_n_seq and clu_read_ids. The queue-based abamd_flat_hb_consensus is
 * compared as a second witness.
 *
 * Built against gpu_stub.c so the aligner is the injected oracle
 * (ABPOA_AMD_TEST_ALIGNER_SO). Prints "cons twin OK (...)" on success; exits
 * non-zero on the first difference. */
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

static void die(const char *what, int read_i, int pos) {
    fprintf(stderr, "CONS TWIN MISMATCH after read %d at %d: %s\n", read_i, pos, what);
    exit(1);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s reads.fa [-r1]\n", argv[0]); return 2; }
    abpoa_para_t *abpt = abpoa_init_para();
    if (argc > 2 && strcmp(argv[2], "-r1") == 0) abpt->out_msa = 1; /* read-id tracking on */
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
    int rid_n = abpt->use_read_ids ? 1 + ((n_seq - 1) >> 6) : 0;
    flat_graph_t fg;
    abamd_flat_init(&fg, total_len + 2, 4 * total_len + 64, 8 * total_len + 1024, rid_n);

    const int cap = total_len + 2;
    int *w = (int*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1) * sizeof(int));
    int *qmap_live = (int*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1) * sizeof(int));
    int *qmap_flat = (int*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1) * sizeof(int));
    uint8_t *codes = (uint8_t*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1));
    for (i = 0; i < max_len; ++i) w[i] = 1;
    /* derived arrays + consensus workspaces, sized like the device slab's
     * per-node regions */
    int *i2n = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *n2i = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *rem = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *scr = (int*)abamd_calloc((size_t)2 * cap, sizeof(int));
    int *max_w = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *best = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *score = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *path = (int*)abamd_calloc((size_t)cap, sizeof(int)); /* becomes cons ids in place */
    int *cov = (int*)abamd_calloc((size_t)cap, sizeof(int));
    uint8_t *bases = (uint8_t*)abamd_calloc((size_t)cap, 1);
    int *q_score = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *q_mout = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *q_id = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *q_cov = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *q_phred = (int*)abamd_calloc((size_t)cap, sizeof(int));
    uint8_t *q_base = (uint8_t*)abamd_calloc((size_t)cap, 1);
    int stage[3 * ABAMD_CONS_CHUNK];
    long checked_bases = 0;
    int max_rows = 0;

    for (i = 0; i < n_seq; ++i) {
        int qlen = abs->seq[i].l;
        for (j = 0; j < qlen; ++j) codes[j] = (uint8_t)ab_amd_char26_table[(int)abs->seq[i].s[j]];
        abpoa_res_t res; memset(&res, 0, sizeof(res));
        abpoa_align_sequence_to_graph(ab, abpt, codes, qlen, &res);
        abamd_flat_apply_alignment(&fg, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, codes, w, qlen,
                                   qmap_flat, res.n_cigar, res.graph_cigar, i,
                                   abpt->use_read_ids, 1);
        abpoa_add_graph_alignment(ab, abpt, codes, w, qlen, qmap_live, res, i, n_seq, 1);
        if (res.n_cigar) free(res.graph_cigar);
        /* derived passes in the fold kernel's order: index BFS on the
         * pre-sort adjacency, weight sort, remain, span counts */
        abamd_flat_topo_index(&fg, i2n, n2i, scr);
        abamd_flat_sort_adjacency(&fg);
        abamd_flat_remain(&fg, rem, scr);
        abamd_flat_update_n_span(&fg, i2n, n2i, 1);
        if (fg.node_n != ab->abg->node_n) die("node_n", i, fg.node_n);
        if (n2i[ABPOA_SINK_NODE_ID] + 1 > max_rows) max_rows = n2i[ABPOA_SINK_NODE_ID] + 1;

        /* 1. phased shared-body consensus over the flat graph + i2n/n2i */
        int clen = -1;
        int status = abamd_flat_cons_phased(&fg, i2n, n2i, max_w, best, score, path,
                                            path /* ids in place, as on the device */,
                                            bases, cov, stage, &clen, 0, 1);
        if (status != ABAMD_CONS_OK) die("phased consensus status", i, status);
        /* 2. the result builder the resident driver uses */
        abpoa_cons_t built; memset(&built, 0, sizeof(built));
        abamd_cons_from_path(&built, n_seq, clen, path, bases, cov);
        /* 3. every field vs the live pointer-graph consensus */
        abpoa_clean_msa_cons(ab);
        ab->abg->is_called_cons = 0;
        abpoa_generate_consensus(ab, abpt);
        const abpoa_cons_t *abc = ab->abc;
        int k;
        if (built.n_cons != abc->n_cons || abc->n_cons != 1) die("n_cons", i, built.n_cons);
        if (built.n_seq != abc->n_seq) die("n_seq", i, built.n_seq);
        if (built.cons_len[0] != abc->cons_len[0]) die("cons_len", i, built.cons_len[0]);
        if (built.clu_n_seq[0] != abc->clu_n_seq[0]) die("clu_n_seq", i, built.clu_n_seq[0]);
        for (k = 0; k < abc->clu_n_seq[0]; ++k)
            if (built.clu_read_ids[0][k] != abc->clu_read_ids[0][k]) die("clu_read_ids", i, k);
        for (k = 0; k < abc->cons_len[0]; ++k) {
            if (built.cons_node_ids[0][k] != abc->cons_node_ids[0][k]) die("cons node id", i, k);
            if (built.cons_base[0][k] != abc->cons_base[0][k]) die("cons base", i, k);
            if (built.cons_cov[0][k] != abc->cons_cov[0][k]) die("cons cov", i, k);
            if (built.cons_phred_score[0][k] != abc->cons_phred_score[0][k]) die("cons phred", i, k);
        }
        /* second witness: the queue-based flat core */
        int qlen2 = abamd_flat_hb_consensus(&fg, n_seq, scr, q_score, q_mout,
                                            q_id, q_base, q_cov, q_phred);
        if (qlen2 != clen) die("queue core cons_len", i, qlen2);
        for (k = 0; k < clen; ++k) {
            if (q_id[k] != built.cons_node_ids[0][k]) die("queue core node id", i, k);
            if (q_base[k] != built.cons_base[0][k]) die("queue core base", i, k);
            if (q_cov[k] != built.cons_cov[0][k]) die("queue core cov", i, k);
            if (q_phred[k] != built.cons_phred_score[0][k]) die("queue core phred", i, k);
        }
        checked_bases += clen;
        abamd_cons_clear(&built);
        abpoa_clean_msa_cons(ab);
        ab->abg->is_called_cons = 0;
    }
    printf("cons twin OK (%d reads, %d nodes, max %d rows, %ld consensus bases compared)\n",
           n_seq, fg.node_n, max_rows, checked_bases);
    free(w); free(qmap_live); free(qmap_flat); free(codes);
    free(i2n); free(n2i); free(rem); free(scr);
    free(max_w); free(best); free(score); free(path); free(cov); free(bases);
    free(q_score); free(q_mout); free(q_id); free(q_cov); free(q_phred); free(q_base);
    abamd_flat_free(&fg);
    abamd_seq_destroy(abs);
    abpoa_free(ab);
    abpoa_free_para(abpt);
    return 0;
}

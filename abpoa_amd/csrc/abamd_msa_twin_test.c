/* MSA-twin test driver: replays every read of a FASTA through the
 * pointer-based graph fold (abamd_graph.c) and the flat-array device-layout
 * core (abamd_fold_core.c) and, after EVERY read, runs the two-stage flat
 * row-column MSA (abamd_msa_core.inc :: abamd_flat_msa_rank_cols and
 * abamd_flat_msa_place — the bodies of the device MSA kernels, here with one
 * lane) over the flat graph, with the consensus ids and bases of the phased
 * flat consensus as the consensus row, exactly as the device-resident driver
 * chains them. msa_len and every row byte are compared against
 * abpoa_generate_rc_msa on the live pointer graph, once with the consensus
 * row (out_cons = 1) and once without (out_cons = 0). The matrix is also
 * attached through abamd_cons_attach_msa (the driver's result builder) and
 * compared row by row.
 *
 * Built against gpu_stub.c so the aligner is the injected oracle
 * (ABPOA_AMD_TEST_ALIGNER_SO). Prints "msa twin OK (...)" on success; exits
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
    fprintf(stderr, "MSA TWIN MISMATCH after read %d at %d: %s\n", read_i, pos, what);
    exit(1);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s reads.fa\n", argv[0]); return 2; }
    abpoa_para_t *abpt = abpoa_init_para();
    abpt->out_msa = 1; /* read-id tracking on */
    abpoa_post_set_para(abpt);
    abpoa_t *ab = abpoa_init();
    abpoa_reset(ab, abpt, 1024);

    abpoa_seq_t *abs = abamd_seq_new();
    abamd_fx_t *fx = abamd_fx_open(argv[1]);
    if (!fx) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n_seq = abamd_read_seq(abs, fx);
    abamd_fx_close(fx);
    ab->abs->n_seq = n_seq;

    int total_len = 0, max_len = 0, i, j, k;
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
    /* derived arrays + workspaces, sized exactly like the device slab's
     * per-node regions: node_n ints each, nothing to spare */
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
    int cstage[3 * ABAMD_CONS_CHUNK];
    int mstage[2];
    long checked_bytes = 0;
    int max_cols = 0;
    const uint8_t gap = (uint8_t)abpt->m;

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
        /* derived passes in the fold kernel's order */
        abamd_flat_topo_index(&fg, i2n, n2i, scr);
        abamd_flat_sort_adjacency(&fg);
        abamd_flat_remain(&fg, rem, scr);
        abamd_flat_update_n_span(&fg, i2n, n2i, 1);
        if (fg.node_n != ab->abg->node_n) die("node_n", i, fg.node_n);

        /* 1. device order: consensus first, its ids/bases stay in place */
        int clen = -1;
        if (abamd_flat_cons_phased(&fg, i2n, n2i, max_w, best, score, path, path, bases, cov,
                                   cstage, &clen, 0, 1) != ABAMD_CONS_OK)
            die("phased consensus status", i, 0);

        /* 2. stage 1 of the MSA in workspaces of exactly node_n ints */
        const int nn = fg.node_n;
        int *rank = (int*)abamd_malloc((size_t)nn * sizeof(int));
        int *col = (int*)abamd_malloc((size_t)nn * sizeof(int));
        int *in_deg = (int*)abamd_malloc((size_t)nn * sizeof(int));
        int *stack = (int*)abamd_malloc((size_t)nn * sizeof(int));
        int msa_len = -1;
        int status = abamd_flat_msa_rank_cols(&fg, rank, col, in_deg, stack, mstage, &msa_len, 0, 1);
        if (status != ABAMD_MSA_OK) die("msa rank status", i, status);
        if (msa_len > max_cols) max_cols = msa_len;

        int with_cons;
        for (with_cons = 1; with_cons >= 0; --with_cons) {
            const int n_rows = n_seq + with_cons;
            /* 3. stage 2 into an exact-size gap-filled matrix */
            uint8_t *mat = (uint8_t*)abamd_malloc((size_t)n_rows * msa_len);
            memset(mat, gap, (size_t)n_rows * msa_len);
            status = abamd_flat_msa_place(&fg, col, n_seq, msa_len, mat, path, bases,
                                          with_cons ? clen : -1, mstage, 0, 1);
            if (status != ABAMD_MSA_OK) die("msa place status", i, status);
            /* 4. the reference rows on the live pointer graph */
            abpoa_clean_msa_cons(ab);
            ab->abg->is_called_cons = 0;
            ab->abg->is_set_msa_rank = 0;
            abpt->out_cons = with_cons;
            abpoa_generate_rc_msa(ab, abpt);
            const abpoa_cons_t *abc = ab->abc;
            if (abc->msa_len != msa_len) die("msa_len", i, msa_len);
            if (abc->n_seq != n_seq) die("n_seq", i, abc->n_seq);
            if (abc->n_cons != with_cons) die("n_cons", i, abc->n_cons);
            for (k = 0; k < n_rows; ++k)
                for (j = 0; j < msa_len; ++j)
                    if (mat[(size_t)k * msa_len + j] != abc->msa_base[k][j]) die("msa byte", i, k * msa_len + j);
            checked_bytes += (long)n_rows * msa_len;
            /* 5. the result builder the resident driver uses: consensus
             * from the path, then the rows attached (read rows only when
             * the consensus row was not built) */
            abpoa_cons_t built; memset(&built, 0, sizeof(built));
            abamd_cons_from_path(&built, n_seq, clen, path, bases, cov);
            abamd_cons_attach_msa(&built, n_rows, msa_len, mat, gap);
            if (built.msa_len != msa_len) die("attached msa_len", i, built.msa_len);
            for (k = 0; k < n_seq + built.n_cons; ++k)
                for (j = 0; j < msa_len; ++j) {
                    const uint8_t want = k < n_rows ? abc->msa_base[k][j] : gap;
                    if (built.msa_base[k][j] != want) die("attached msa byte", i, k * msa_len + j);
                }
            abamd_cons_clear(&built);
            free(mat);
        }
        abpt->out_cons = 1;
        abpoa_clean_msa_cons(ab);
        ab->abg->is_called_cons = 0;
        ab->abg->is_set_msa_rank = 0;
        free(rank); free(col); free(in_deg); free(stack);
    }
    printf("msa twin OK (%d reads, %d nodes, %d words, max %d columns, %ld matrix bytes compared)\n",
           n_seq, fg.node_n, rid_n, max_cols, checked_bytes);
    free(w); free(qmap_live); free(qmap_flat); free(codes);
    free(i2n); free(n2i); free(rem); free(scr);
    free(max_w); free(best); free(score); free(path); free(cov); free(bases);
    abamd_flat_free(&fg);
    abamd_seq_destroy(abs);
    abpoa_free(ab);
    abpoa_free_para(abpt);
    return 0;
}

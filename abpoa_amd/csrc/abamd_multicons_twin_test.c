/* Multi-consensus twin test driver: replays every read of a FASTA through the
 * pointer-based graph fold (abamd_graph.c) and the flat-array device-layout
 * core (abamd_fold_core.c) and, after EVERY read, runs the device
 * multi-consensus stage of the resident batch driver with one lane over the
 * flat graph, in the driver's order and in workspaces mapped as the driver
 * maps them:
 *   rank/place (abamd_flat_msa_rank_cols, abamd_flat_msa_place, cons_len -1),
 *   the het scan (abamd_flat_het_count into the dead rank array,
 *   abamd_flat_het_gather), abamd_read_clu_from_msa on the compact matrix,
 *   abamd_flat_cons_phased_clu per cluster (abamd_flat_cons_phased for one
 *   cluster), with -r2 abamd_flat_msa_place_cons_row per cluster, and the
 *   result builders abamd_cons_from_paths / abamd_cons_from_path +
 *   abamd_cons_attach_msa.
 * The result is compared field by field against abpoa_generate_consensus on
 * the live pointer graph (with -r2 abpoa_generate_rc_msa): n_cons, clu_n_seq,
 * clu_read_ids, cons_len, node ids, bases, coverage, phred, and with -r2
 * msa_len and every row, consensus rows included. Two more comparisons: the
 * candidate list against a brute-force count over the matrix, and the
 * clusters from the compact matrix against those from the full one.
 *
 * --mutate FIELD (n_cons, clu_read_ids, cons_base, cons_cov, cons_row) changes
 * that field of the built result after the last read, before the comparison:
 * the run must then exit with status 1 and name the field.
 *
 * Built against gpu_stub.c so the aligner is the injected oracle
 * (ABPOA_AMD_TEST_ALIGNER_SO). Prints "multicons twin OK (...)" on success. */
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

extern uint64_t abamd_clu_path_counts[2]; /* abamd_cons.c */

static void die(const char *field, int read_i, int pos) {
    printf("MULTICONS TWIN MISMATCH after read %d at %d: field %s\n", read_i, pos, field);
    exit(1);
}

int main(int argc, char **argv) {
    const char *fa = NULL, *mutate = NULL;
    int ploidy = 2, with_rows = 0, a;
    for (a = 1; a < argc; ++a) {
        if (strcmp(argv[a], "-d") == 0 && a + 1 < argc) ploidy = atoi(argv[++a]);
        else if (strncmp(argv[a], "-d", 2) == 0 && argv[a][2]) ploidy = atoi(argv[a] + 2);
        else if (strcmp(argv[a], "-r2") == 0) with_rows = 1;
        else if (strcmp(argv[a], "--mutate") == 0 && a + 1 < argc) mutate = argv[++a];
        else if (!fa) fa = argv[a];
        else fa = "";
    }
    if (!fa || !*fa || ploidy < 2) {
        fprintf(stderr, "usage: %s reads.fa -d N [-r2] [--mutate FIELD]\n", argv[0]);
        return 2;
    }
    if (mutate && strcmp(mutate, "n_cons") && strcmp(mutate, "clu_read_ids") &&
        strcmp(mutate, "cons_base") && strcmp(mutate, "cons_cov") && strcmp(mutate, "cons_row")) {
        fprintf(stderr, "unknown --mutate field %s\n", mutate);
        return 2;
    }
    if (mutate && !strcmp(mutate, "cons_row") && !with_rows) {
        fprintf(stderr, "--mutate cons_row needs -r2\n");
        return 2;
    }
    abpoa_para_t *abpt = abpoa_init_para();
    abpt->max_n_cons = ploidy;
    if (with_rows) { abpt->out_msa = 1; abpt->out_cons = 1; }
    abpoa_post_set_para(abpt);
    if (!abpt->use_read_ids || abpt->m > ABAMD_HET_MAX_M) { fprintf(stderr, "configuration not eligible\n"); return 2; }
    abpoa_t *ab = abpoa_init();
    abpoa_reset(ab, abpt, 1024);

    abpoa_seq_t *abs = abamd_seq_new();
    abamd_fx_t *fx = abamd_fx_open(fa);
    if (!fx) { fprintf(stderr, "cannot open %s\n", fa); return 2; }
    int n_seq = abamd_read_seq(abs, fx);
    abamd_fx_close(fx);
    ab->abs->n_seq = n_seq;

    int total_len = 0, max_len = 0, i, j, k, c;
    for (i = 0; i < n_seq; ++i) {
        total_len += abs->seq[i].l;
        if (abs->seq[i].l > max_len) max_len = abs->seq[i].l;
    }
    const int rid_n = 1 + ((n_seq - 1) >> 6);
    flat_graph_t fg;
    abamd_flat_init(&fg, total_len + 2, 4 * total_len + 64, 8 * total_len + 1024, rid_n);

    const int cap = total_len + 2;
    int *w = (int*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1) * sizeof(int));
    int *qmap_live = (int*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1) * sizeof(int));
    int *qmap_flat = (int*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1) * sizeof(int));
    uint8_t *codes = (uint8_t*)abamd_malloc((size_t)(max_len > 0 ? max_len : 1));
    for (i = 0; i < max_len; ++i) w[i] = 1;
    int *i2n = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *n2i = (int*)abamd_calloc((size_t)cap, sizeof(int));
    /* the slab regions the driver uses: scratch (2 x node_cap: in-degree +
     * stack, then max_w + best), pre_off (rank, then the candidate list),
     * out_off (col, kept to the end), row_node_id (score), row_remain (path /
     * cons ids), max_left (coverage), max_right (bases) */
    int *scr = (int*)abamd_calloc((size_t)2 * cap, sizeof(int));
    int *pre_off = (int*)abamd_calloc((size_t)cap + 1, sizeof(int));
    int *out_off = (int*)abamd_calloc((size_t)cap + 1, sizeof(int));
    int *row_node_id = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *row_remain = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *max_left = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int *max_right = (int*)abamd_calloc((size_t)cap, sizeof(int));
    int cstage[3 * ABAMD_CONS_CHUNK];
    int hstage[ABAMD_HET_STAGE];
    int mstage[2];
    const uint8_t gap = (uint8_t)abpt->m;
    const int extra_rows = with_rows ? ploidy : 0;
    long cand_total = 0, clusters_total = 0, bases_total = 0, row_bytes = 0;
    int max_clu_seen = 0, mutated = 0;

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
        abamd_flat_update_n_span(&fg, i2n, n2i, 1);
        if (fg.node_n != ab->abg->node_n) die("node_n", i, fg.node_n);
        const int nn = fg.node_n;

        /* 1. ranks and columns */
        int *rank = pre_off, *col = out_off, msa_len = -1;
        int status = abamd_flat_msa_rank_cols(&fg, rank, col, scr, scr + cap, mstage, &msa_len, 0, 1);
        if (status != ABAMD_MSA_OK) die("msa rank status", i, status);

        /* 2. read rows, with room for the consensus rows */
        const size_t mat_rows = (size_t)n_seq + extra_rows;
        uint8_t *mat = (uint8_t*)abamd_malloc(mat_rows * msa_len);
        memset(mat, gap, mat_rows * msa_len);
        status = abamd_flat_msa_place(&fg, col, n_seq, msa_len, mat, NULL, NULL, -1, mstage, 0, 1);
        if (status != ABAMD_MSA_OK) die("msa place status", i, status);

        /* 3. het scan; the candidate list takes the dead rank array */
        int min_het, min_hom, n_cand = -1, *cand = pre_off;
        abamd_het_depth_bounds(n_seq, abpt, &min_het, &min_hom);
        status = abamd_flat_het_count(mat, n_seq, msa_len, abpt->m, min_het, min_hom, cand, cap,
                                      hstage, &n_cand, 0, 1);
        if (status != ABAMD_MSA_OK) die("het count status", i, status);
        {   /* brute force over the matrix, column by column */
            int n_bf = 0;
            for (j = 0; j < msa_len; ++j) {
                int n_uniq = 0, s;
                for (s = 0; s <= abpt->m; ++s) {
                    int d = 0;
                    for (k = 0; k < n_seq; ++k) d += mat[(size_t)k * msa_len + j] == s;
                    if (d >= min_het && d <= min_hom) ++n_uniq;
                }
                if (n_uniq < 2) continue;
                if (n_bf >= n_cand || cand[n_bf] != j) die("candidate list", i, j);
                ++n_bf;
            }
            if (n_bf != n_cand) die("candidate count", i, n_cand);
        }
        uint8_t *compact = (uint8_t*)abamd_malloc((size_t)n_seq * (n_cand > 0 ? n_cand : 1));
        status = abamd_flat_het_gather(mat, n_seq, msa_len, cand, n_cand, compact, mstage, 0, 1);
        if (status != ABAMD_MSA_OK) die("het gather status", i, status);
        cand_total += n_cand;

        /* 4. clusters from the compact matrix, and from the full one */
        uint8_t **rows = (uint8_t**)abamd_malloc((size_t)n_seq * sizeof(uint8_t*));
        uint64_t **clu = NULL, **clu_full = NULL;
        int n_clu = 1, n_clu_full;
        if (n_cand > 0) {
            for (k = 0; k < n_seq; ++k) rows[k] = compact + (size_t)k * n_cand;
            n_clu = abamd_read_clu_from_msa(rows, n_cand, n_seq, abpt, &clu);
        }
        for (k = 0; k < n_seq; ++k) rows[k] = mat + (size_t)k * msa_len;
        n_clu_full = abamd_read_clu_from_msa(rows, msa_len, n_seq, abpt, &clu_full);
        if (n_clu != n_clu_full) die("clusters compact vs full: count", i, n_clu);
        if (n_clu > 1)
            for (c = 0; c < n_clu; ++c)
                if (memcmp(clu[c], clu_full[c], 8 * (size_t)rid_n)) die("clusters compact vs full: mask", i, c);
        if (n_clu > max_clu_seen) max_clu_seen = n_clu;
        clusters_total += n_clu;

        /* 5 + 6. consensus per cluster, its row placed before the next pass
         * reuses the workspaces */
        abpoa_cons_t built; memset(&built, 0, sizeof(built));
        int *max_w = scr, *best = scr + cap, *score = row_node_id, *path = row_remain;
        int *cov = max_left;
        uint8_t *bases = (uint8_t*)max_right;
        if (n_clu == 1) {
            int clen = -1;
            status = abamd_flat_cons_phased(&fg, i2n, n2i, max_w, best, score, path, path, bases, cov,
                                            cstage, &clen, 0, 1);
            if (status != ABAMD_CONS_OK) die("phased consensus status", i, status);
            abamd_cons_from_path(&built, n_seq, clen, path, bases, cov);
            if (with_rows) {
                status = abamd_flat_msa_place_cons_row(nn, col, msa_len, mat + (size_t)n_seq * msa_len,
                                                       path, bases, clen, mstage, 0, 1);
                if (status != ABAMD_MSA_OK) die("cons row status", i, status);
            }
        } else {
            uint64_t *masks = (uint64_t*)abamd_malloc(8 * (size_t)n_clu * rid_n);
            int *lens = (int*)abamd_malloc((size_t)n_clu * sizeof(int));
            int **ids = (int**)abamd_malloc((size_t)n_clu * sizeof(int*));
            int **covs = (int**)abamd_malloc((size_t)n_clu * sizeof(int*));
            uint8_t **bss = (uint8_t**)abamd_malloc((size_t)n_clu * sizeof(uint8_t*));
            for (c = 0; c < n_clu; ++c) {
                int clen = -1;
                memcpy(masks + (size_t)c * rid_n, clu[c], 8 * (size_t)rid_n);
                status = abamd_flat_cons_phased_clu(&fg, masks + (size_t)c * rid_n, i2n, n2i, max_w, best,
                                                    score, path, path, bases, cov, cstage, &clen, 0, 1);
                if (status != ABAMD_CONS_OK) die("phased cluster consensus status", i, c);
                lens[c] = clen;
                ids[c] = (int*)abamd_malloc((size_t)(clen + 1) * sizeof(int));
                covs[c] = (int*)abamd_malloc((size_t)(clen + 1) * sizeof(int));
                bss[c] = (uint8_t*)abamd_malloc((size_t)clen + 1);
                memcpy(ids[c], path, (size_t)clen * sizeof(int));
                memcpy(covs[c], cov, (size_t)clen * sizeof(int));
                memcpy(bss[c], bases, (size_t)clen);
                if (with_rows) {
                    status = abamd_flat_msa_place_cons_row(nn, col, msa_len,
                                                           mat + (size_t)(n_seq + c) * msa_len,
                                                           path, bases, clen, mstage, 0, 1);
                    if (status != ABAMD_MSA_OK) die("cons row status", i, c);
                }
            }
            abamd_cons_from_paths(&built, n_seq, n_clu, masks, lens, (const int *const *)ids,
                                  (const uint8_t *const *)bss, (const int *const *)covs);
            for (c = 0; c < n_clu; ++c) { free(ids[c]); free(covs[c]); free(bss[c]); }
            free(masks); free(lens); free(ids); free(covs); free(bss);
        }
        if (with_rows) abamd_cons_attach_msa(&built, n_seq + n_clu, msa_len, mat, gap);

        /* the mutation, once, on the final graph */
        if (mutate && i == n_seq - 1) {
            if (!strcmp(mutate, "n_cons")) { built.n_cons += 1; mutated = 1; }
            else if (!strcmp(mutate, "clu_read_ids") && built.clu_n_seq[0] > 0) { built.clu_read_ids[0][0] ^= 1; mutated = 1; }
            else if (!strcmp(mutate, "cons_base") && built.cons_len[0] > 0) {
                built.cons_base[0][0] = (uint8_t)((built.cons_base[0][0] + 1) % 4); mutated = 1;
            } else if (!strcmp(mutate, "cons_cov") && built.cons_len[0] > 0) { built.cons_cov[0][0] += 1; mutated = 1; }
            else if (!strcmp(mutate, "cons_row") && built.msa_len > 0) {
                uint8_t *row = built.msa_base[n_seq + built.n_cons - 1];
                row[msa_len / 2] = (uint8_t)(row[msa_len / 2] == gap ? 0 : gap); mutated = 1;
            }
        }

        /* 7. every field against the live pointer graph */
        abpoa_clean_msa_cons(ab);
        ab->abg->is_called_cons = 0;
        ab->abg->is_set_msa_rank = 0;
        if (with_rows) abpoa_generate_rc_msa(ab, abpt);
        else abpoa_generate_consensus(ab, abpt);
        const abpoa_cons_t *abc = ab->abc;
        if (built.n_cons != abc->n_cons) die("n_cons", i, built.n_cons);
        if (abc->n_cons != n_clu) die("n_cons vs clusters", i, n_clu);
        if (built.n_seq != abc->n_seq) die("n_seq", i, built.n_seq);
        for (c = 0; c < abc->n_cons; ++c) {
            if (built.clu_n_seq[c] != abc->clu_n_seq[c]) die("clu_n_seq", i, c);
            for (k = 0; k < abc->clu_n_seq[c]; ++k)
                if (built.clu_read_ids[c][k] != abc->clu_read_ids[c][k]) die("clu_read_ids", i, k);
            if (built.cons_len[c] != abc->cons_len[c]) die("cons_len", i, c);
            for (k = 0; k < abc->cons_len[c]; ++k) {
                if (built.cons_node_ids[c][k] != abc->cons_node_ids[c][k]) die("cons_node_ids", i, k);
                if (built.cons_base[c][k] != abc->cons_base[c][k]) die("cons_base", i, k);
                if (built.cons_cov[c][k] != abc->cons_cov[c][k]) die("cons_cov", i, k);
                if (built.cons_phred_score[c][k] != abc->cons_phred_score[c][k]) die("cons_phred", i, k);
            }
            bases_total += abc->cons_len[c];
        }
        if (with_rows) {
            if (built.msa_len != abc->msa_len || msa_len != abc->msa_len) die("msa_len", i, built.msa_len);
            for (k = 0; k < n_seq + abc->n_cons; ++k)
                for (j = 0; j < msa_len; ++j)
                    if (built.msa_base[k][j] != abc->msa_base[k][j])
                        die(k < n_seq ? "msa read row" : "cons_row", i, k * msa_len + j);
            row_bytes += (long)(n_seq + abc->n_cons) * msa_len;
        }
        abamd_cons_clear(&built);
        abpoa_clean_msa_cons(ab);
        ab->abg->is_called_cons = 0;
        ab->abg->is_set_msa_rank = 0;
        if (clu) { for (c = 0; c < n_clu; ++c) free(clu[c]); free(clu); }
        if (n_clu_full > 1) { for (c = 0; c < n_clu_full; ++c) free(clu_full[c]); free(clu_full); }
        free(rows); free(compact); free(mat);
    }
    if (mutate) {
        fprintf(stderr, mutated ? "--mutate %s went unnoticed\n" : "--mutate %s never applied\n", mutate);
        return 2;
    }
    printf("clustering paths: wide-partition %llu short-seed %llu\n",
           (unsigned long long)abamd_clu_path_counts[0], (unsigned long long)abamd_clu_path_counts[1]);
    {   /* the final clusters' sizes, for the tests that pin them */
        abpoa_generate_consensus(ab, abpt);
        printf("clusters");
        for (c = 0; c < ab->abc->n_cons; ++c) printf(" %d", ab->abc->clu_n_seq[c]);
        printf("\n");
    }
    printf("multicons twin OK (%d reads, %d nodes, -d%d, max %d clusters, %ld clusters, "
           "%ld candidate columns, %ld consensus bases, %ld row bytes compared)\n",
           n_seq, fg.node_n, ploidy, max_clu_seen, clusters_total, cand_total, bases_total, row_bytes);
    free(w); free(qmap_live); free(qmap_flat); free(codes);
    free(i2n); free(n2i); free(scr);
    free(pre_off); free(out_off); free(row_node_id); free(row_remain); free(max_left); free(max_right);
    abamd_flat_free(&fg);
    abamd_seq_destroy(abs);
    abpoa_free(ab);
    abpoa_free_para(abpt);
    return 0;
}

/* CPU self-test of the per-round fold check (abamd_fold_round_check.c), in
 * the pattern of abpoa_amd_seamtwin: the "device" is a second flat twin,
 * advanced by the same serial passes from the injected oracle's CIGARs
 * (ABPOA_AMD_TEST_ALIGNER_SO), handed to the comparison through the same
 * abpoa_amd_fold_probe_t the resident driver fills. Unchanged it must pass;
 * with --mutate NAME@READ one thing in the copy handed over at that read is
 * changed, and the comparison must name it:
 *   out_order    two neighbouring equal-weight out-edges swapped in a chain
 *   out_tail     a node's out_tail left at its first edge
 *   rem          max_remain of one prefix node off by one
 *   n_span_read  of one node off by one
 *   pre_off      one entry shifted
 *   pre_idx      two entries of one row swapped
 *   row_remain   one entry changed
 *   n_out        the record's n_out changed
 *
 * Usage: abpoa_amd_foldroundtwin [--mutate NAME@READ] [-r1] reads.fa
 * Prints the checker's summary line and "fold-round twin OK (...)", or the
 * checker's MISMATCH line and exits 1; a mutation that found no place to
 * apply exits 2. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"
#include "abamd_fold_core.h"
#include "abamd_fold_round_check.h"

typedef struct abamd_fx_t abamd_fx_t;
abpoa_seq_t *abamd_seq_new(void);
void abamd_seq_destroy(abpoa_seq_t *abs);
abamd_fx_t *abamd_fx_open(const char *fn);
void abamd_fx_close(abamd_fx_t *x);
int abamd_read_seq(abpoa_seq_t *abs, abamd_fx_t *x);

static int *dup_ints(const int *src, size_t n) {
    int *d = (int*)abamd_malloc((n ? n : 1) * sizeof(int));
    if (n) memcpy(d, src, n * sizeof(int));
    return d;
}

int main(int argc, char **argv) {
    const char *mut = NULL, *fa = NULL;
    int mut_read = -1, r1 = 0, a;
    for (a = 1; a < argc; ++a) {
        if (strcmp(argv[a], "--mutate") == 0 && a + 1 < argc) {
            char *at = strchr(argv[++a], '@');
            if (!at) { fprintf(stderr, "--mutate NAME@READ\n"); return 2; }
            *at = 0; mut = argv[a]; mut_read = atoi(at + 1);
        } else if (strcmp(argv[a], "-r1") == 0) r1 = 1;
        else fa = argv[a];
    }
    if (!fa) { fprintf(stderr, "usage: %s [--mutate NAME@READ] [-r1] reads.fa\n", argv[0]); return 2; }

    abpoa_para_t *abpt = abpoa_init_para();
    if (r1) abpt->out_msa = 1; /* read-id tracking on */
    abpoa_post_set_para(abpt);
    const int use_remain = abpt->wb >= 0 || abpt->zdrop > 0;
    abpoa_t *ab = abpoa_init();
    abpoa_reset(ab, abpt, 1024);

    abpoa_seq_t *abs = abamd_seq_new();
    abamd_fx_t *fx = abamd_fx_open(fa);
    if (!fx) { fprintf(stderr, "cannot open %s\n", fa); return 2; }
    int n_seq = abamd_read_seq(abs, fx);
    abamd_fx_close(fx);
    ab->abs->n_seq = n_seq;

    int i, j, total_len = 0, max_len = 1;
    int *lens = (int*)abamd_calloc(n_seq ? n_seq : 1, sizeof(int));
    uint8_t **seqs = (uint8_t**)abamd_calloc(n_seq ? n_seq : 1, sizeof(uint8_t*));
    for (i = 0; i < n_seq; ++i) {
        lens[i] = abs->seq[i].l;
        total_len += lens[i];
        if (lens[i] > max_len) max_len = lens[i];
        seqs[i] = (uint8_t*)abamd_malloc(lens[i] ? lens[i] : 1);
        for (j = 0; j < lens[i]; ++j) seqs[i][j] = (uint8_t)ab_amd_char26_table[(int)abs->seq[i].s[j]];
    }
    const int *lens_p = lens;
    const uint8_t *const *seqs_p = (const uint8_t *const *)seqs;
    abamd_frc_t *frc = abamd_frc_new(abpt, 1, &n_seq, &lens_p, &seqs_p);

    /* the "device": same capacities the checker's twin plans */
    const int rid_n = abpt->use_read_ids ? 1 + ((n_seq - 1) >> 6) : 0;
    const int nc = total_len + 2 + 8, ec = total_len + n_seq + 8, ac = 2 * abpt->m * total_len + 1024;
    flat_graph_t dg;
    abamd_flat_init(&dg, nc, ec, ac, rid_n);
    int *i2n = (int*)abamd_calloc(nc, sizeof(int)), *n2i = (int*)abamd_calloc(nc, sizeof(int));
    int *rem = (int*)abamd_calloc(nc, sizeof(int)), *scr = (int*)abamd_calloc(2 * (size_t)nc, sizeof(int));
    uint8_t *row_base = (uint8_t*)abamd_calloc(nc, 1);
    int *row_node_id = (int*)abamd_calloc(nc, sizeof(int));
    int *pre_off = (int*)abamd_calloc((size_t)nc + 1, sizeof(int));
    int *out_off = (int*)abamd_calloc((size_t)nc + 1, sizeof(int));
    int *row_remain = (int*)abamd_calloc(nc, sizeof(int));
    int *pre_idx = (int*)abamd_calloc(ec, sizeof(int)), *out_idx = (int*)abamd_calloc(ec, sizeof(int));
    int *w = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    for (i = 0; i < max_len; ++i) w[i] = 1;

    int applied = 0, rc = 0;
    for (i = 0; i < n_seq && !rc; ++i) {
        abpoa_res_t res; memset(&res, 0, sizeof(res));
        abpoa_align_sequence_to_graph(ab, abpt, seqs[i], lens[i], &res);
        abamd_flat_apply_alignment(&dg, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, seqs[i], w, lens[i],
                                   NULL, res.n_cigar, res.graph_cigar, i, abpt->use_read_ids, 1);
        abamd_flat_topo_index(&dg, i2n, n2i, scr);
        abamd_flat_sort_adjacency(&dg);
        abamd_flat_remain(&dg, rem, scr);
        abamd_flat_update_n_span(&dg, i2n, n2i, 1);
        const int n_rows = abamd_flat_build_rows(&dg, i2n, n2i, rem, use_remain, row_base, row_node_id,
                                                 pre_off, out_off, row_remain, pre_idx, out_idx);

        abpoa_amd_fold_probe_t p;
        memset(&p, 0, sizeof(p));
        p.set_idx = 0; p.read_idx = i;
        p.status = ABPOA_AMD_FOLD_PROBE_OK;
        p.walk = p.out.walk = 0;
        p.use_remain = use_remain;
        p.node_cap = nc; p.edge_cap = ec; p.aln_cap = ac; p.rid_n = rid_n;
        p.out.node_n = dg.node_n; p.out.edge_n_in = dg.edge_n_in; p.out.edge_n_out = dg.edge_n_out;
        p.out.aln_n = dg.aln_n;
        p.out.n_rows = n_rows; p.out.n_pre = pre_off[n_rows]; p.out.n_out = out_off[n_rows];
        p.n_cigar = res.n_cigar; p.cigar = res.n_cigar ? (const uint64_t*)res.graph_cigar : NULL;
        p.base = dg.base; p.n_read = dg.n_read; p.n_span_read = dg.n_span_read;
        p.in_head = dg.in_head; p.in_tail = dg.in_tail; p.out_head = dg.out_head;
        p.out_tail = dg.out_tail; p.aln_head = dg.aln_head;
        p.in_to = dg.in_to; p.in_w = dg.in_w; p.in_next = dg.in_next;
        p.out_to = dg.out_to; p.out_w = dg.out_w; p.out_next = dg.out_next;
        p.rid_pool = dg.rid_pool; p.aln_id = dg.aln_id; p.aln_next = dg.aln_next;
        p.i2n = i2n; p.n2i = n2i; p.rem = rem;
        p.row_base = row_base; p.row_node_id = row_node_id; p.pre_off = pre_off; p.out_off = out_off;
        p.row_remain = row_remain; p.pre_idx = pre_idx; p.out_idx = out_idx;

        int *m1 = NULL, *m2 = NULL, *m3 = NULL; /* mutated copies, freed below */
        if (mut && i == mut_read) {
            const int n = dg.node_n;
            int k, e;
            if (strcmp(mut, "out_order") == 0) {
                m1 = dup_ints(dg.out_head, n); m2 = dup_ints(dg.out_next, dg.edge_n_out);
                m3 = dup_ints(dg.out_tail, n);
                for (k = 0; k < n && !applied; ++k) {
                    int prev = -1;
                    for (e = dg.out_head[k]; e != -1 && dg.out_next[e] != -1; prev = e, e = dg.out_next[e]) {
                        const int f = dg.out_next[e];
                        if (dg.out_w[e] != dg.out_w[f]) continue;
                        /* prev -> e -> f -> rest  becomes  prev -> f -> e -> rest */
                        if (prev == -1) m1[k] = f; else m2[prev] = f;
                        m2[e] = dg.out_next[f]; m2[f] = e;
                        if (m3[k] == f) m3[k] = e;
                        applied = 1;
                        break;
                    }
                }
                p.out_head = m1; p.out_next = m2; p.out_tail = m3;
            } else if (strcmp(mut, "out_tail") == 0) {
                m1 = dup_ints(dg.out_tail, n);
                for (k = 0; k < n && !applied; ++k)
                    if (dg.out_head[k] != -1 && dg.out_head[k] != dg.out_tail[k]) {
                        m1[k] = dg.out_head[k]; applied = 1;
                    }
                p.out_tail = m1;
            } else if (strcmp(mut, "rem") == 0) {
                m1 = dup_ints(rem, n);
                if (use_remain) { m1[i2n[n_rows / 2]] += 1; applied = 1; }
                p.rem = m1;
            } else if (strcmp(mut, "n_span_read") == 0) {
                m1 = dup_ints(dg.n_span_read, n);
                m1[n - 1] -= 1; applied = 1;
                p.n_span_read = m1;
            } else if (strcmp(mut, "pre_off") == 0) {
                m1 = dup_ints(pre_off, (size_t)n_rows + 1);
                m1[n_rows / 2] += 1; applied = 1;
                p.pre_off = m1;
            } else if (strcmp(mut, "pre_idx") == 0) {
                m1 = dup_ints(pre_idx, pre_off[n_rows]);
                for (k = 1; k < n_rows && !applied; ++k)
                    if (pre_off[k + 1] - pre_off[k] >= 2) {
                        int t = m1[pre_off[k]]; m1[pre_off[k]] = m1[pre_off[k] + 1]; m1[pre_off[k] + 1] = t;
                        applied = 1;
                    }
                p.pre_idx = m1;
            } else if (strcmp(mut, "row_remain") == 0) {
                m1 = dup_ints(row_remain, n_rows);
                m1[n_rows - 2] += 1; applied = 1;
                p.row_remain = m1;
            } else if (strcmp(mut, "n_out") == 0) {
                p.out.n_out += 1; applied = 1;
            } else {
                fprintf(stderr, "unknown mutation %s\n", mut);
                return 2;
            }
        }
        rc = abamd_frc_check(frc, &p, stdout);
        free(m1); free(m2); free(m3);

        abpoa_add_graph_alignment(ab, abpt, seqs[i], w, lens[i], NULL, res, i, n_seq, 1);
        if (res.n_cigar) free(res.graph_cigar);
    }
    if (mut && !applied) {
        fprintf(stderr, "mutation %s@%d never applied (no such read, or no place for it)\n", mut, mut_read);
        rc = 2;
    } else {
        abamd_frc_summary(frc, stdout);
        if (rc) printf("fold-round twin FAILED\n");
        else printf("fold-round twin OK (%d reads, %d nodes, %d out-edges)\n", n_seq, dg.node_n, dg.edge_n_out);
    }

    abamd_frc_free(frc);
    abamd_flat_free(&dg);
    free(i2n); free(n2i); free(rem); free(scr); free(row_base); free(row_node_id);
    free(pre_off); free(out_off); free(row_remain); free(pre_idx); free(out_idx); free(w);
    for (i = 0; i < n_seq; ++i) free(seqs[i]);
    free(seqs); free(lens);
    abamd_seq_destroy(abs);
    abpoa_free(ab);
    abpoa_free_para(abpt);
    return rc;
}

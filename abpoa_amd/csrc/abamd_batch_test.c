/* Test tool: run the batched multi-set driver over N FASTA files (one read
 * set per file) and print each set's consensus, one ">set_N" record per set.
 * Before the file list it takes the CLI's options with the CLI's spelling and
 * effect (abamd_cliopts.c: -m -M -X -O -E -b -f -z -e -c -t ...). -r1
 * (row-column MSA, out_cons off) or -r2 (consensus plus MSA) sets
 * abpt->out_msa; each ">set_N" record is then followed by the set's MSA rows,
 * one per line: the read rows, then with -r2 the consensus rows. Without the
 * option the output is unchanged.
 *
 * -S (here, unlike the CLI's seeding switch, which means nothing to the
 * batched driver) prints one more line to stderr after the records:
 *   [batch-stats] key=value ...
 * with the counters of abpoa_amd_get_batch_stats, the fold-walk counts and the
 * device/host/fallback set counts of the consensus and MSA stages, and the DP
 * cells and plane bytes of abpoa_amd_get_stats/_stats2, so a test can prove
 * which path of the driver its input took.
 *
 * --fold-check (anywhere before the files; abpoa_amd_batchgpu only) installs
 * a fold probe (abpoa_amd_batch_set_fold_probe) and checks what the production
 * fold kernel wrote after EVERY fold of every set against a host twin advanced
 * by the serial abamd_flat_* passes (abamd_fold_round_check.c): counters,
 * pools, chains with heads and tails, read-id bitsets, topological order,
 * max_remain and the seven DP-row CSR arrays. The first difference is named on
 * stderr (set, read, field, index) and the exit status is 1 once the batch
 * call has returned; a "[fold-check] ..." summary line goes to stderr either
 * way (tests/test_fold_round_gpu.py).
 *
 * Two programs are built from this file:
 *   abpoa_amd_batchtest  linked with gpu_stub.o: the host-fold driver, with
 *                        the alignments routed through the dispatch seam, where
 *                        tests inject the oracle via ABPOA_AMD_TEST_ALIGNER_SO.
 *                        Exists so the pipeline driver's item ordering (groups,
 *                        lookahead, big-item fallback) is exercised on CPU-only
 *                        machines too. Parity requirement: output must be
 *                        byte-identical across ABPOA_AMD_GROUPS=1/2/3 and equal
 *                        to the sequential CLI consensus (and -r1/-r2 rows) on
 *                        each file.
 *   abpoa_amd_batchgpu   linked with the GPU core: the device-resident driver
 *                        (tests/test_resident_paths_gpu.py). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"
#include "abamd_fold_round_check.h"

/* forward-declared file-local seq API (abamd_seq.c) */
typedef struct abamd_fx_t abamd_fx_t;
abpoa_seq_t *abamd_seq_new(void);
void abamd_seq_destroy(abpoa_seq_t *abs);
abamd_fx_t *abamd_fx_open(const char *fn);
void abamd_fx_close(abamd_fx_t *x);
int abamd_read_seq(abpoa_seq_t *abs, abamd_fx_t *x);

int abamd_cli_parse_opts(int argc, char **argv, abpoa_para_t *abpt, int *in_list, int *harness_stats);
extern int optind;

typedef struct { char **cons; char **msa; int n; int out_msa, out_cons; } out_t;

static void cb(int set_idx, const abpoa_cons_t *cons, void *user) {
    out_t *o = (out_t*)user;
    /* the rows are only valid during the callback: copy them out as text */
    if (o->out_msa && cons->msa_len > 0 && cons->msa_base) {
        const int rows = cons->n_seq + (o->out_cons ? cons->n_cons : 0);
        char *m = (char*)malloc((size_t)rows * ((size_t)cons->msa_len + 1) + 1), *p = m;
        for (int r = 0; r < rows; ++r) {
            for (int i = 0; i < cons->msa_len; ++i)
                *p++ = ab_amd_char256_table[cons->msa_base[r][i]];
            *p++ = '\n';
        }
        *p = 0;
        o->msa[set_idx] = m;
    }
    if (cons->n_cons < 1) { o->cons[set_idx] = strdup(""); return; }
    char *s = (char*)malloc((size_t)cons->cons_len[0] + 1);
    for (int i = 0; i < cons->cons_len[0]; ++i)
        s[i] = ab_amd_char256_table[cons->cons_base[0][i]];
    s[cons->cons_len[0]] = 0;
    o->cons[set_idx] = s;
}

static void print_stats(void) {
    uint64_t b[10], f[3], c[5], m[5], cells = 0, alg_bytes = 0;
    abpoa_amd_get_stats(&cells, NULL, NULL);
    abpoa_amd_get_stats2(&alg_bytes);
    abpoa_amd_get_batch_stats(&b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &b[7], &b[8], &b[9]);
    abpoa_amd_get_fold_stats(&f[0], &f[1], &f[2]);
    abpoa_amd_get_cons_stats(&c[0], &c[1], &c[2], &c[3], &c[4]);
    abpoa_amd_get_msa_stats(&m[0], &m[1], &m[2], &m[3], &m[4]);
    fprintf(stderr, "[batch-stats] resident_calls=%llu hostfold_calls=%llu dp_retry_jobs=%llu "
                    "dp_retry_launches=%llu pool_expands=%llu big_chunks=%llu noop_folds=%llu "
                    "seam_retry_jobs=%llu launches_i16=%llu launches_i32=%llu "
                    "parallel_folds=%llu fallback_folds=%llu serial_folds=%llu "
                    "cons_device_sets=%llu cons_host_sets=%llu cons_fallback_sets=%llu "
                    "msa_device_sets=%llu msa_host_sets=%llu msa_fallback_sets=%llu "
                    "dp_cells=%llu alg_bytes=%llu\n",
            (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)b[2],
            (unsigned long long)b[3], (unsigned long long)b[4], (unsigned long long)b[5],
            (unsigned long long)b[6], (unsigned long long)b[7], (unsigned long long)b[8],
            (unsigned long long)b[9],
            (unsigned long long)f[0], (unsigned long long)f[1], (unsigned long long)f[2],
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
            (unsigned long long)m[0], (unsigned long long)m[1], (unsigned long long)m[2],
            (unsigned long long)cells, (unsigned long long)alg_bytes);
}

static void fold_probe(const abpoa_amd_fold_probe_t *p, void *user) {
    abamd_frc_check((abamd_frc_t*)user, p, stderr);
}

int main(int argc, char **argv) {
    int stats = 0, rc, fold_check = 0;
    abpoa_para_t *abpt = abpoa_init_para();
    {   /* the one long option: take it out before getopt sees it */
        int i, k = 1;
        for (i = 1; i < argc; ++i) {
            if (strcmp(argv[i], "--fold-check") == 0) fold_check = 1;
            else argv[k++] = argv[i];
        }
        argc = k;
        argv[argc] = NULL;
    }
    rc = abamd_cli_parse_opts(argc, argv, abpt, NULL, &stats);
    if (rc < 0) return 0;
    if (rc > 0 || argc - optind < 1) {
        fprintf(stderr, "usage: %s [CLI alignment options] [-r1|-r2] [-S] [--fold-check] set1.fa [set2.fa ...]\n", argv[0]);
        return 2;
    }
    const int arg0 = optind, out_msa = abpt->out_msa, out_cons = abpt->out_cons;
    int n_sets = argc - arg0;
    abpoa_post_set_para(abpt); /* after the options: out_msa switches read ids on */

    int *n_seqs = (int*)abamd_calloc(n_sets, sizeof(int));
    int **lens = (int**)abamd_calloc(n_sets, sizeof(int*));
    uint8_t ***seqs = (uint8_t***)abamd_calloc(n_sets, sizeof(uint8_t**));
    for (int s = 0; s < n_sets; ++s) {
        abpoa_seq_t *abs = abamd_seq_new();
        abamd_fx_t *fx = abamd_fx_open(argv[s + arg0]);
        if (!fx) { fprintf(stderr, "cannot open %s\n", argv[s + arg0]); return 2; }
        n_seqs[s] = abamd_read_seq(abs, fx);
        abamd_fx_close(fx);
        lens[s] = (int*)abamd_calloc(n_seqs[s], sizeof(int));
        seqs[s] = (uint8_t**)abamd_calloc(n_seqs[s], sizeof(uint8_t*));
        for (int i = 0; i < n_seqs[s]; ++i) {
            int l = abs->seq[i].l;
            lens[s][i] = l;
            seqs[s][i] = (uint8_t*)abamd_malloc(l);
            for (int j = 0; j < l; ++j)
                seqs[s][i][j] = (uint8_t)ab_amd_char26_table[(uint8_t)abs->seq[i].s[j]];
        }
        abamd_seq_destroy(abs);
    }
    out_t out; out.n = n_sets; out.out_msa = out_msa; out.out_cons = out_cons;
    out.cons = (char**)abamd_calloc(n_sets, sizeof(char*));
    out.msa = (char**)abamd_calloc(n_sets, sizeof(char*));
    abamd_frc_t *frc = NULL;
    if (fold_check) {
        frc = abamd_frc_new(abpt, n_sets, n_seqs, (const int *const *)lens,
                            (const uint8_t *const *const *)seqs);
        abpoa_amd_batch_set_fold_probe(fold_probe, frc);
    }
    abpoa_amd_msa_batch(abpt, n_sets, n_seqs,
                        (const int *const *)lens,
                        (const uint8_t *const *const *)seqs, cb, &out, 4);
    abpoa_amd_batch_set_fold_probe(NULL, NULL);
    for (int s = 0; s < n_sets; ++s) {
        printf(">set_%d\n%s\n", s, out.cons[s] ? out.cons[s] : "");
        if (out.msa[s]) fputs(out.msa[s], stdout);
    }
    if (stats) { fflush(stdout); print_stats(); }
    if (frc) {
        uint64_t b[2];
        fflush(stdout);
        abamd_frc_summary(frc, stderr);
        abpoa_amd_get_batch_stats(&b[0], &b[1], NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
        if (abamd_frc_failed(frc)) return 1;
        if (b[0] == 0) {
            /* the host-fold driver has no fold kernel: nothing was checked */
            fprintf(stderr, "--fold-check: the device-resident driver did not serve this call\n");
            return 3;
        }
    }
    return 0;
}

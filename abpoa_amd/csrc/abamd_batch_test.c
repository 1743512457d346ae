/* Test tool: run the batched multi-set driver over N FASTA files (one read
 * set per file) and print each set's consensus, one ">set_N" record per set.
 * An optional leading -r1 (row-column MSA, out_cons off) or -r2 (consensus
 * plus MSA) sets abpt->out_msa; each ">set_N" record is then followed by the
 * set's MSA rows, one per line: the read rows, then with -r2 the consensus
 * rows. Without the option the output is unchanged.
 *
 * Exists so the pipeline driver's item ordering (groups, lookahead, big-item
 * fallback) is exercised on CPU-only machines too: built against gpu_stub.c
 * the alignments route through the dispatch seam, where tests inject the
 * oracle via ABPOA_AMD_TEST_ALIGNER_SO. Parity requirement: output must be
 * byte-identical across ABPOA_AMD_GROUPS=1/2/3 and equal to the sequential
 * CLI consensus (and -r1/-r2 rows) on each file. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"

/* forward-declared file-local seq API (abamd_seq.c) */
typedef struct abamd_fx_t abamd_fx_t;
abpoa_seq_t *abamd_seq_new(void);
void abamd_seq_destroy(abpoa_seq_t *abs);
abamd_fx_t *abamd_fx_open(const char *fn);
void abamd_fx_close(abamd_fx_t *x);
int abamd_read_seq(abpoa_seq_t *abs, abamd_fx_t *x);

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
        s[i] = "ACGTN"[cons->cons_base[0][i]];
    s[cons->cons_len[0]] = 0;
    o->cons[set_idx] = s;
}

int main(int argc, char **argv) {
    int arg0 = 1, out_msa = 0, out_cons = 1;
    if (argc > 1 && strcmp(argv[1], "-r1") == 0) { out_msa = 1; out_cons = 0; arg0 = 2; }
    else if (argc > 1 && strcmp(argv[1], "-r2") == 0) { out_msa = 1; arg0 = 2; }
    if (argc - arg0 < 1) { fprintf(stderr, "usage: %s [-r1|-r2] set1.fa [set2.fa ...]\n", argv[0]); return 2; }
    int n_sets = argc - arg0;
    abpoa_para_t *abpt = abpoa_init_para();
    if (out_msa) { abpt->out_msa = 1; abpt->out_cons = out_cons; } /* before post_set: read ids on */
    abpoa_post_set_para(abpt);

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
                seqs[s][i][j] = ab_amd_nt4_table[(uint8_t)abs->seq[i].s[j]];
        }
        abamd_seq_destroy(abs);
    }
    out_t out; out.n = n_sets; out.out_msa = out_msa; out.out_cons = out_cons;
    out.cons = (char**)abamd_calloc(n_sets, sizeof(char*));
    out.msa = (char**)abamd_calloc(n_sets, sizeof(char*));
    abpoa_amd_msa_batch(abpt, n_sets, n_seqs,
                        (const int *const *)lens,
                        (const uint8_t *const *const *)seqs, cb, &out, 4);
    for (int s = 0; s < n_sets; ++s) {
        printf(">set_%d\n%s\n", s, out.cons[s] ? out.cons[s] : "");
        if (out.msa[s]) fputs(out.msa[s], stdout);
    }
    return 0;
}

/* Seam differential harness: the aligner seam's abpoa_res_t, field by field.
 *
 * Replays the per-read loop of abamd_msa.c over one or more FASTA/FASTQ files
 * and, for every read after the one that seeds the graph, aligns it twice on
 * the SAME abpoa_t in one process: with the scalar oracle
 * (oracle_align_sequence_to_subgraph, dlopen'ed from the path given as the
 * first argument) and with the device under test. Each side fills a freshly
 * zeroed abpoa_res_t; best_score, n_cigar, every packed CIGAR word, node_s/e,
 * query_s/e, n_aln_bases and n_matched_bases are compared. The ORACLE's result
 * is folded into the graph, so one divergence does not cascade.
 *
 * Two programs are built from this file:
 *   abpoa_amd_seamgpu   (-DABAMD_SEAM_GPU, linked with the GPU core): the
 *                       device under test is abamd_gpu_align_sequence_to_subgraph
 *   abpoa_amd_seamtwin  (linked with gpu_stub.o, runs without a GPU): the
 *                       device under test is the oracle behind a mutator
 *                       (--mutate FIELD@READ) that changes exactly one thing,
 *                       which proves that the comparator can fail.
 *
 * The oracle keeps the adaptive band state in the graph's max_pos arrays and
 * relies on abpoa_topological_sort having reset them; the GPU core keeps that
 * state on the device. Several alignments run here per sort, so the harness
 * re-applies the sort's reset before every oracle call.
 *
 * Usage: PROG liboracle.so [scoring/band flags] [mode flags] in.fa [in2.fa ...]
 *   -m -M -X -O -E -b -f -z -e -G -R -J -Q -c -t   as in the CLI
 *   --settings       GPU aligns three times per read: default,
 *                    ABPOA_AMD_DP_GENERIC=1, ABPOA_AMD_DP_RING=1
 *   --windows N      N subgraph alignments per read as well, between matched
 *                    nodes of the oracle's CIGAR widened by abpoa_subgraph_nodes
 *   --no-cigar       ret_cigar = 0 (best_score and n_cigar == 0 compared)
 *   --rev-cigar      rev_cigar = 1
 *   --both-strands   also align the reverse complement of every read
 *   --batch          (GPU) afterwards one abamd_gpu_align_batch call with one
 *                    job per input file against that file's final graph
 *   --cells          per whole-graph alignment one line "seam cells read R: rows N
 *                    qlen Q oracle C est E n_cigar K": the oracle's banded cells per
 *                    plane against the arena reservation of the product drivers,
 *                    rows * (2w + 160) + qlen + 64 (job_est_cells in
 *                    gpu_batch_resident.cpp, pack_job in gpu_align.cpp)
 *   --mutate F@R     (twin) F in best_score n_cigar node_s node_e query_s
 *                    query_e n_aln_bases n_matched_bases cigar_op cigar_node
 *                    cigar_query cigar_last, applied to read R's whole-graph
 *                    alignment
 * Prints at most 20 mismatches, goes on to the end, and exits 1 if there was
 * one. Before the last line it prints the longest insertion among the oracle's
 * CIGAR words and, in the GPU program, the score width the host picked for
 * each alignment (abamd_pick_width) and how many convex alignments went to the
 * fast and to the generic instantiation (abamd_cg_fast_eligible and
 * abamd_dp_force_generic, as gpu_align.cpp asks them). Last line: "seam OK: R reads, A alignments, W cigar words compared". */
#include <dlfcn.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"

typedef struct abamd_fx_t abamd_fx_t;
abpoa_seq_t *abamd_seq_new(void);
void abamd_seq_destroy(abpoa_seq_t *abs);
abamd_fx_t *abamd_fx_open(const char *fn);
void abamd_fx_close(abamd_fx_t *x);
int abamd_read_seq(abpoa_seq_t *abs, abamd_fx_t *x);

#ifdef ABAMD_SEAM_GPU
int abamd_gpu_align_sequence_to_subgraph(abpoa_t *ab, abpoa_para_t *abpt,
        int beg_node_id, int end_node_id, uint8_t *query, int qlen, abpoa_res_t *res);
void abamd_pick_width(abpoa_para_t *abpt, int qlen, int gn, int *bits, int *inf_min);
int abamd_dp_ring_depth(void);
int abamd_dp_force_generic(void);
int abamd_cg_fast_eligible(int align_mode, int banded, int inc_path_score, int dp_ring);
/* must match gpu_align.cpp's BatchJob */
typedef struct {
    abpoa_t *ab; abpoa_para_t *abpt;
    int beg_node_id, end_node_id;
    uint8_t *query; int qlen; abpoa_res_t *res;
    int64_t est_cells_hint; int64_t *cells_out;
} seam_batch_job_t;
int abamd_gpu_align_batch(seam_batch_job_t *batch, int n_jobs);
#endif

static abpoa_amd_aligner_fn g_oracle;

#define MAX_REPORT 20
static long g_reads, g_alns, g_words, g_mismatches, g_longest_ins;
#ifdef ABAMD_SEAM_GPU
static long g_n16, g_n32, g_fast, g_generic;
#endif

static int opt_settings, opt_windows, opt_both, opt_batch, opt_cells;
static void (*g_oracle_cells)(int64_t *cells, int64_t *rows);
static char *mut_field; static int mut_read = -1, mut_applied;

static const char *const SETTING_NAME[3] = { "default", "ABPOA_AMD_DP_GENERIC=1", "ABPOA_AMD_DP_RING=1" };

static void apply_setting(int s) {
    unsetenv("ABPOA_AMD_DP_GENERIC"); unsetenv("ABPOA_AMD_DP_RING");
    if (s == 1) setenv("ABPOA_AMD_DP_GENERIC", "1", 1);
    else if (s == 2) setenv("ABPOA_AMD_DP_RING", "1", 1);
}

/* what abpoa_topological_sort leaves in the band state (abamd_graph.c) */
static void reset_band(abpoa_t *ab, abpoa_para_t *abpt) {
    abpoa_graph_t *g = ab->abg; int i;
    if (abpt->wb < 0) return;
    for (i = 0; i < g->node_n; ++i) {
        g->node_id_to_max_pos_right[i] = 0;
        g->node_id_to_max_pos_left[i] = g->node_n;
    }
}

static void mismatch(int read_i, const char *what, const char *setting, const char *field,
                     long long o, long long d) {
    if (g_mismatches++ < MAX_REPORT)
        printf("seam MISMATCH read %d (%s, %s) field %s: oracle %lld device %lld\n",
               read_i, what, setting, field, o, d);
}

static void decode(abpoa_cigar_t w, char *buf, size_t n) {
    int op = (int)(w & 0xf); long long hi = (long long)(w >> 34), mid = (long long)((w >> 4) & 0x3fffffff);
    char c = op < 6 ? ABPOA_CIGAR_STR[op] : '?';
    if (op == ABPOA_CMATCH || op == ABPOA_CDIFF) snprintf(buf, n, "%c node %lld query %lld", c, hi, mid);
    else if (op == ABPOA_CDEL) snprintf(buf, n, "%c node %lld len %lld", c, hi, mid);
    else snprintf(buf, n, "%c query %lld len %lld", c, hi, mid);
}

static void compare(abpoa_para_t *abpt, int read_i, const char *what, const char *setting,
                    const abpoa_res_t *o, const abpoa_res_t *d) {
    ++g_alns;
    if (o->best_score != d->best_score) mismatch(read_i, what, setting, "best_score", o->best_score, d->best_score);
    if (!abpt->ret_cigar) {
        if (d->n_cigar != 0) mismatch(read_i, what, setting, "n_cigar", 0, d->n_cigar);
        return;
    }
    if (o->n_cigar != d->n_cigar) mismatch(read_i, what, setting, "n_cigar", o->n_cigar, d->n_cigar);
    int i, n = o->n_cigar < d->n_cigar ? o->n_cigar : d->n_cigar;
    for (i = 0; i < n; ++i) {
        ++g_words;
        abpoa_cigar_t a = o->graph_cigar[i], b = d->graph_cigar[i];
        if ((a & 0xf) == ABPOA_CINS && (long)((a >> 4) & 0x3fffffff) > g_longest_ins)
            g_longest_ins = (long)((a >> 4) & 0x3fffffff);
        if (a == b) continue;
        if (g_mismatches++ < MAX_REPORT) {
            char sa[96], sb[96]; decode(a, sa, sizeof(sa)); decode(b, sb, sizeof(sb));
            int op = (int)(a & 0xf);
            const char *hi = (op == ABPOA_CMATCH || op == ABPOA_CDIFF || op == ABPOA_CDEL) ? "node" : "query";
            const char *mid = (op == ABPOA_CMATCH || op == ABPOA_CDIFF) ? "query" : "len";
            printf("seam MISMATCH read %d (%s, %s) field cigar[%d] of %d:%s%s%s%s%s differs: oracle 0x%llx (%s) device 0x%llx (%s)\n",
                   read_i, what, setting, i, o->n_cigar,
                   (a & 0xf) != (b & 0xf) ? " op" : "",
                   (a >> 34) != (b >> 34) ? " " : "", (a >> 34) != (b >> 34) ? hi : "",
                   ((a >> 4) & 0x3fffffff) != ((b >> 4) & 0x3fffffff) ? " " : "",
                   ((a >> 4) & 0x3fffffff) != ((b >> 4) & 0x3fffffff) ? mid : "",
                   (unsigned long long)a, sa, (unsigned long long)b, sb);
        }
    }
    if (o->node_s != d->node_s) mismatch(read_i, what, setting, "node_s", o->node_s, d->node_s);
    if (o->node_e != d->node_e) mismatch(read_i, what, setting, "node_e", o->node_e, d->node_e);
    if (o->query_s != d->query_s) mismatch(read_i, what, setting, "query_s", o->query_s, d->query_s);
    if (o->query_e != d->query_e) mismatch(read_i, what, setting, "query_e", o->query_e, d->query_e);
    if (o->n_aln_bases != d->n_aln_bases) mismatch(read_i, what, setting, "n_aln_bases", o->n_aln_bases, d->n_aln_bases);
    if (o->n_matched_bases != d->n_matched_bases) mismatch(read_i, what, setting, "n_matched_bases", o->n_matched_bases, d->n_matched_bases);
}

#ifndef ABAMD_SEAM_GPU
/* change exactly one thing in the device-under-test side */
static void mutate(abpoa_res_t *d) {
    const char *f = mut_field; int i, mid = -1;
    mut_applied = 1;
    if (!strcmp(f, "best_score")) { d->best_score += 1; return; }
    if (!strcmp(f, "n_cigar")) { d->n_cigar -= 1; return; }
    if (!strcmp(f, "node_s")) { d->node_s += 1; return; }
    if (!strcmp(f, "node_e")) { d->node_e += 1; return; }
    if (!strcmp(f, "query_s")) { d->query_s += 1; return; }
    if (!strcmp(f, "query_e")) { d->query_e += 1; return; }
    if (!strcmp(f, "n_aln_bases")) { d->n_aln_bases += 1; return; }
    if (!strcmp(f, "n_matched_bases")) { d->n_matched_bases += 1; return; }
    if (d->n_cigar <= 0) abamd_fatal("seam", "--mutate %s: the alignment has no CIGAR", f);
    if (!strcmp(f, "cigar_last")) { d->graph_cigar[d->n_cigar - 1] += (abpoa_cigar_t)1 << 4; return; }
    /* the match word nearest the middle */
    for (i = 0; i < d->n_cigar; ++i)
        if ((d->graph_cigar[i] & 0xf) == ABPOA_CMATCH &&
            (mid < 0 || abs(i - d->n_cigar / 2) < abs(mid - d->n_cigar / 2))) mid = i;
    if (mid < 0) abamd_fatal("seam", "--mutate %s: the CIGAR has no match word", f);
    if (!strcmp(f, "cigar_op")) d->graph_cigar[mid] ^= (abpoa_cigar_t)ABPOA_CDIFF; /* M -> X */
    else if (!strcmp(f, "cigar_node")) d->graph_cigar[mid] += (abpoa_cigar_t)1 << 34;
    else if (!strcmp(f, "cigar_query")) d->graph_cigar[mid] += (abpoa_cigar_t)1 << 4;
    else abamd_fatal("seam", "--mutate: unknown field '%s'", f);
}
#endif

/* Align query to [beg,end] with the oracle and with the device under test
 * (once per setting), compare, and hand the oracle's result to the caller. */
static abpoa_res_t align_pair(abpoa_t *ab, abpoa_para_t *abpt, int beg_id, int end_id,
                              uint8_t *q, int qlen, int read_i, const char *what, int whole) {
    abpoa_res_t ro; memset(&ro, 0, sizeof(ro));
    reset_band(ab, abpt);
    g_oracle(ab, abpt, beg_id, end_id, q, qlen, &ro);
    if (opt_cells && whole) {
        int64_t cells = 0, rows = 0;
        g_oracle_cells(&cells, &rows);
        int w = abpt->wb < 0 ? qlen : abpt->wb + (int)(abpt->wf * qlen);
        printf("seam cells read %d: rows %lld qlen %d oracle %lld est %lld n_cigar %d\n", read_i, (long long)rows, qlen,
               (long long)cells, (long long)(rows * (2 * (int64_t)w + 160) + qlen + 64), ro.n_cigar);
    }
    int s, n_set = opt_settings ? 3 : 1;
    for (s = 0; s < n_set; ++s) {
        abpoa_res_t rd; memset(&rd, 0, sizeof(rd));
        if (opt_settings) apply_setting(s);
#ifdef ABAMD_SEAM_GPU
        {
            abpoa_graph_t *g = ab->abg; int bits, inf_min;
            abamd_pick_width(abpt, qlen, g->node_id_to_index[end_id] - g->node_id_to_index[beg_id] + 1, &bits, &inf_min);
            if (bits == 16) ++g_n16; else ++g_n32;
            if (abpt->gap_mode == ABPOA_CONVEX_GAP) {
                if (!abamd_dp_force_generic() &&
                    abamd_cg_fast_eligible(abpt->align_mode, abpt->wb >= 0, abpt->inc_path_score, abamd_dp_ring_depth()))
                    ++g_fast;
                else ++g_generic;
            }
        }
        abamd_gpu_align_sequence_to_subgraph(ab, abpt, beg_id, end_id, q, qlen, &rd);
#else
        reset_band(ab, abpt);
        g_oracle(ab, abpt, beg_id, end_id, q, qlen, &rd);
        if (mut_field && whole && read_i == mut_read && s == 0) mutate(&rd);
#endif
        compare(abpt, read_i, what, opt_settings ? SETTING_NAME[s] : "default", &ro, &rd);
        if (rd.graph_cigar) free(rd.graph_cigar);
    }
    if (opt_settings) apply_setting(0);
    return ro;
}

/* N subgraph alignments between matched nodes of the oracle's CIGAR */
static void align_windows(abpoa_t *ab, abpoa_para_t *abpt, uint8_t *q, int read_i, const abpoa_res_t *ro) {
    int i, k = 0, t, N = opt_windows;
    if (ro->n_cigar <= 0) return;
    int *node = (int*)abamd_malloc((size_t)ro->n_cigar * sizeof(int));
    int *qpos = (int*)abamd_malloc((size_t)ro->n_cigar * sizeof(int));
    for (i = 0; i < ro->n_cigar; ++i) {
        /* query order whichever way the CIGAR runs */
        abpoa_cigar_t w = ro->graph_cigar[abpt->rev_cigar ? ro->n_cigar - 1 - i : i];
        if ((w & 0xf) != ABPOA_CMATCH) continue;
        node[k] = (int)(w >> 34); qpos[k] = (int)((w >> 4) & 0x3fffffff); ++k;
    }
    for (t = 0; t < N && k >= 2 * (N + 1); ++t) {
        int a = t * k / (N + 1), b = (t + 2) * k / (N + 1) - 1, eb, ee;
        char what[32]; snprintf(what, sizeof(what), "window %d", t);
        abpoa_subgraph_nodes(ab, abpt, node[a], node[b], &eb, &ee);
        abpoa_res_t r = align_pair(ab, abpt, eb, ee, q + qpos[a], qpos[b] - qpos[a] + 1, read_i, what, 0);
        if (r.graph_cigar) free(r.graph_cigar);
    }
    free(node); free(qpos);
}

typedef struct { abpoa_t *ab; uint8_t *last; int last_l; } seam_file_t;

static void run_file(const char *fn, abpoa_para_t *abpt, seam_file_t *out) {
    abpoa_t *ab = abpoa_init();
    abpoa_reset(ab, abpt, 1024);
    abpoa_seq_t *abs = abamd_seq_new();
    abamd_fx_t *fx = abamd_fx_open((char*)fn);
    if (!fx) abamd_fatal("seam", "cannot open %s", fn);
    int n_seq = abamd_read_seq(abs, fx), i, j;
    abamd_fx_close(fx);
    if (n_seq <= 0) abamd_fatal("seam", "no reads in %s", fn);
    ab->abs->n_seq = n_seq;
    int max_len = 1;
    for (i = 0; i < n_seq; ++i) if (abs->seq[i].l > max_len) max_len = abs->seq[i].l;
    uint8_t *q = (uint8_t*)abamd_malloc((size_t)max_len), *rc = (uint8_t*)abamd_malloc((size_t)max_len);
    int *w = (int*)abamd_malloc((size_t)max_len * sizeof(int));
    for (i = 0; i < n_seq; ++i, ++g_reads) {
        int qlen = abs->seq[i].l;
        for (j = 0; j < qlen; ++j) q[j] = (uint8_t)ab_amd_char26_table[(int)abs->seq[i].s[j]];
        for (j = 0; j < qlen; ++j)
            w[j] = (abpt->use_qv && abs->qual[i].l > 0) ? (int)abs->qual[i].s[j] - 32 : 1;
        abpoa_res_t res; memset(&res, 0, sizeof(res));
        if (ab->abg->node_n > 2) {
            if (ab->abg->is_topological_sorted == 0) abpoa_topological_sort(ab->abg, abpt);
            res = align_pair(ab, abpt, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, q, qlen, i, "whole graph", 1);
            if (opt_windows) align_windows(ab, abpt, q, i, &res);
            if (opt_both) {
                for (j = 0; j < qlen; ++j) rc[j] = q[qlen - j - 1] < 4 ? (uint8_t)(3 - q[qlen - j - 1]) : 4;
                abpoa_res_t r = align_pair(ab, abpt, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, rc, qlen, i, "reverse strand", 0);
                if (r.graph_cigar) free(r.graph_cigar);
            }
        }
        if (abpt->rev_cigar && res.n_cigar) { /* the fold reads front-to-back order */
            int a, b;
            for (a = 0, b = res.n_cigar - 1; a < b; ++a, --b) {
                abpoa_cigar_t t = res.graph_cigar[a]; res.graph_cigar[a] = res.graph_cigar[b]; res.graph_cigar[b] = t;
            }
        }
        abpoa_add_graph_alignment(ab, abpt, q, w, qlen, NULL, res, i, n_seq, 1);
        if (res.graph_cigar) free(res.graph_cigar);
    }
    out->ab = ab; out->last_l = abs->seq[n_seq - 1].l;
    out->last = (uint8_t*)abamd_malloc((size_t)(out->last_l > 0 ? out->last_l : 1));
    for (j = 0; j < out->last_l; ++j) out->last[j] = (uint8_t)ab_amd_char26_table[(int)abs->seq[n_seq - 1].s[j]];
    free(q); free(rc); free(w);
    abamd_seq_destroy(abs);
}

#ifdef ABAMD_SEAM_GPU
/* one launch, one job per file: each file's last read against its final graph */
static void run_batch(abpoa_para_t *abpt, seam_file_t *files, int n) {
    seam_batch_job_t *jobs = (seam_batch_job_t*)abamd_calloc((size_t)n, sizeof(seam_batch_job_t));
    abpoa_res_t *ro = (abpoa_res_t*)abamd_calloc((size_t)n, sizeof(abpoa_res_t));
    abpoa_res_t *rd = (abpoa_res_t*)abamd_calloc((size_t)n, sizeof(abpoa_res_t));
    int i, launch_bits = 16;
    for (i = 0; i < n; ++i) {
        abpoa_t *ab = files[i].ab; int bits, inf_min;
        if (ab->abg->is_topological_sorted == 0) abpoa_topological_sort(ab->abg, abpt);
        reset_band(ab, abpt);
        g_oracle(ab, abpt, ABPOA_SRC_NODE_ID, ABPOA_SINK_NODE_ID, files[i].last, files[i].last_l, &ro[i]);
        abamd_pick_width(abpt, files[i].last_l, ab->abg->node_n, &bits, &inf_min);
        printf("seam batch job %d: qlen %d, rows %d, picks int%d\n", i, files[i].last_l, ab->abg->node_n, bits);
        if (bits > launch_bits) launch_bits = bits;
        jobs[i].ab = ab; jobs[i].abpt = abpt;
        jobs[i].beg_node_id = ABPOA_SRC_NODE_ID; jobs[i].end_node_id = ABPOA_SINK_NODE_ID;
        jobs[i].query = files[i].last; jobs[i].qlen = files[i].last_l; jobs[i].res = &rd[i];
    }
    printf("seam batch launch: %d jobs at int%d\n", n, launch_bits);
    abamd_gpu_align_batch(jobs, n);
    for (i = 0; i < n; ++i) {
        char what[32]; snprintf(what, sizeof(what), "batch job %d", i);
        compare(abpt, -1, what, "default", &ro[i], &rd[i]);
        if (ro[i].graph_cigar) free(ro[i].graph_cigar);
        if (rd[i].graph_cigar) free(rd[i].graph_cigar);
    }
    free(jobs); free(ro); free(rd);
}
#endif

int main(int argc, char **argv) {
    static const struct option lopts[] = {
        { "settings", no_argument, 0, 1000 }, { "windows", required_argument, 0, 1001 },
        { "no-cigar", no_argument, 0, 1002 }, { "rev-cigar", no_argument, 0, 1003 },
        { "both-strands", no_argument, 0, 1004 }, { "batch", no_argument, 0, 1005 },
        { "mutate", required_argument, 0, 1006 }, { "cells", no_argument, 0, 1007 },
        { 0, 0, 0, 0 } };
    int c, i; char *s;
    abpoa_para_t *abpt = abpoa_init_para();
    while ((c = getopt_long(argc, argv, "m:M:X:O:E:b:f:z:e:GRJQct:", lopts, NULL)) >= 0) {
        switch (c) {
            case 'm': abpt->align_mode = atoi(optarg); break;
            case 'M': abpt->match = atoi(optarg); break;
            case 'X': abpt->mismatch = atoi(optarg); break;
            case 'O': abpt->gap_open1 = (int)strtol(optarg, &s, 10);
                      abpt->gap_open2 = (*s == ',') ? (int)strtol(s + 1, &s, 10) : 0; break;
            case 'E': abpt->gap_ext1 = (int)strtol(optarg, &s, 10);
                      abpt->gap_ext2 = (*s == ',') ? (int)strtol(s + 1, &s, 10) : 0; break;
            case 'b': abpt->wb = atoi(optarg); break;
            case 'f': abpt->wf = (float)atof(optarg); break;
            case 'z': abpt->zdrop = atoi(optarg); break;
            case 'e': abpt->end_bonus = atoi(optarg); break;
            case 'G': abpt->inc_path_score = 1; break;
            case 'R': abpt->put_gap_on_right = 1; break;
            case 'J': abpt->put_gap_at_end = 1; break;
            case 'Q': abpt->use_qv = 1; break;
            case 'c': abpt->m = 27;
                      abpt->mat = (int*)abamd_realloc(abpt->mat, (size_t)abpt->m * abpt->m * sizeof(int)); break;
            case 't': abpt->use_score_matrix = 1; abpt->mat_fn = strdup(optarg); break;
            case 1000: opt_settings = 1; break;
            case 1001: opt_windows = atoi(optarg); break;
            case 1002: abpt->ret_cigar = 0; break;
            case 1003: abpt->rev_cigar = 1; break;
            case 1004: opt_both = 1; break;
            case 1005: opt_batch = 1; break;
            case 1006: mut_field = strdup(optarg); break;
            case 1007: opt_cells = 1; break;
            default: return 2;
        }
    }
    if (argc - optind < 2) {
        fprintf(stderr, "usage: %s liboracle.so [flags] in.fa [in2.fa ...]\n", argv[0]);
        return 2;
    }
    if (mut_field) {
        char *at = strchr(mut_field, '@');
        if (!at) abamd_fatal("seam", "--mutate wants FIELD@READ");
        *at = 0; mut_read = atoi(at + 1);
    }
#ifdef ABAMD_SEAM_GPU
    if (mut_field) abamd_fatal("seam", "--mutate belongs to the twin program");
#else
    if (opt_batch) abamd_fatal("seam", "--batch belongs to the GPU program");
#endif
    if (!abpt->ret_cigar && (opt_windows || mut_field))
        abamd_fatal("seam", "--no-cigar leaves nothing to fold: not with --windows or --mutate");
    abpoa_post_set_para(abpt);
    if (opt_both && abpt->m > 5) abamd_fatal("seam", "--both-strands is for nucleotides");

    const char *so = argv[optind++];
    void *h = dlopen(so, RTLD_NOW | RTLD_LOCAL);
    if (!h) abamd_fatal("seam", "dlopen(%s) failed: %s", so, dlerror());
    g_oracle = (abpoa_amd_aligner_fn)(size_t)dlsym(h, "oracle_align_sequence_to_subgraph");
    if (!g_oracle) abamd_fatal("seam", "oracle_align_sequence_to_subgraph not found in %s", so);

    if (opt_cells) {
        g_oracle_cells = (void (*)(int64_t*, int64_t*))(size_t)dlsym(h, "oracle_last_cells");
        if (!g_oracle_cells) abamd_fatal("seam", "oracle_last_cells not found in %s", so);
    }

    int n_files = argc - optind;
    seam_file_t *files = (seam_file_t*)abamd_calloc((size_t)n_files, sizeof(seam_file_t));
    for (i = 0; i < n_files; ++i) run_file(argv[optind + i], abpt, &files[i]);
#ifdef ABAMD_SEAM_GPU
    if (opt_batch) run_batch(abpt, files, n_files);
    printf("seam widths: int16 %ld, int32 %ld\n", g_n16, g_n32);
    printf("seam convex instantiation: fast %ld, generic %ld\n", g_fast, g_generic);
#endif
    printf("seam longest insertion: %ld\n", g_longest_ins);
    for (i = 0; i < n_files; ++i) { abpoa_free(files[i].ab); free(files[i].last); }
    free(files);
    abpoa_free_para(abpt);
    if (mut_field && !mut_applied) abamd_fatal("seam", "--mutate: read %d was never aligned", mut_read);
    free(mut_field);
    if (g_mismatches) {
        printf("seam FAILED: %ld mismatches (%ld reads, %ld alignments, %ld cigar words compared)\n",
               g_mismatches, g_reads, g_alns, g_words);
        return 1;
    }
    printf("seam OK: %ld reads, %ld alignments, %ld cigar words compared\n", g_reads, g_alns, g_words);
    return 0;
}

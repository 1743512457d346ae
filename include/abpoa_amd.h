/* abpoa_amd — MI355X-native partial order alignment library.
 *
 * Public C ABI. This header mirrors the reference abPOA public interface
 * (yangao07/abPOA include/abpoa.h) so that the library is a drop-in for the
 * hot path: struct layouts and function signatures are field-for-field
 * compatible with the reference (each declaration cites the reference line it
 * replaces), while every implementation behind them is written from scratch
 * for MI355X (HIP/CDNA4 aligner core; clean C host).
 *
 * The aligner seam exported here is exactly the one the reference resolves
 * per-ISA at runtime (abpoa_align_simd.h:11-12, abpoa_dispatch_simd.c:59-82):
 *   simd_abpoa_align_sequence_to_graph / _to_subgraph
 * so reference host code links against this library unchanged.
 */
#ifndef ABPOA_AMD_H
#define ABPOA_AMD_H

#include <stdint.h>
#include <stdio.h>

/* alignment modes (abpoa.h:6-8) */
#define ABPOA_GLOBAL_MODE 0
#define ABPOA_LOCAL_MODE  1
#define ABPOA_EXTEND_MODE 2

/* gap cost models (abpoa.h:12-14) */
#define ABPOA_LINEAR_GAP 0
#define ABPOA_AFFINE_GAP 1
#define ABPOA_CONVEX_GAP 2

/* adaptive band defaults: band half-width = wb + wf*qlen (abpoa.h:16-17) */
#define ABPOA_EXTRA_B 10
#define ABPOA_EXTRA_F 0.01

/* graph-CIGAR operations (abpoa.h:19-25) */
#define ABPOA_CIGAR_STR "MIDXSH"
#define ABPOA_CMATCH     0
#define ABPOA_CINS       1
#define ABPOA_CDEL       2
#define ABPOA_CDIFF      3
#define ABPOA_CSOFT_CLIP 4
#define ABPOA_CHARD_CLIP 5

/* the two virtual terminals of every partial order graph (abpoa.h:27-28) */
#define ABPOA_SRC_NODE_ID  0
#define ABPOA_SINK_NODE_ID 1

/* output selection (abpoa.h:30-35) */
#define ABPOA_OUT_CONS     0
#define ABPOA_OUT_MSA      1
#define ABPOA_OUT_CONS_MSA 2
#define ABPOA_OUT_GFA      3
#define ABPOA_OUT_CONS_GFA 4
#define ABPOA_OUT_CONS_FQ  5

/* consensus algorithms (abpoa.h:37-38) */
#define ABPOA_HB 0
#define ABPOA_MF 1

/* verbosity (abpoa.h:40-43) */
#define ABPOA_NONE_VERBOSE 0
#define ABPOA_INFO_VERBOSE 1
#define ABPOA_DEBUG_VERBOSE 2
#define ABPOA_LONG_DEBUG_VERBOSE 3

/* 64-bit packed graph-CIGAR word (abpoa.h:45-50):
 *   M/X: node_id<<34 | query_id<<4 | op
 *   I/S/H: query_id<<34 | len<<4 | op
 *   D:   node_id<<34 | len<<4 | op            */
#define abpoa_cigar_t uint64_t

#ifdef __cplusplus
extern "C" {
#endif

/* alignment result (abpoa.h:57-64) */
typedef struct {
    int n_cigar, m_cigar; abpoa_cigar_t *graph_cigar;
    int node_s, node_e, query_s, query_e;
    int n_aln_bases, n_matched_bases;
    int32_t best_score;
} abpoa_res_t;

/* parameters (abpoa.h:66-89); field order preserved for ABI compatibility */
typedef struct {
    int m; int *mat; char *mat_fn;
    int use_score_matrix;
    int match, max_mat, mismatch, min_mis, gap_open1, gap_open2, gap_ext1, gap_ext2; int inf_min;
    int sort_input_seq;
    int inc_path_score;
    int k, w, min_w;                 /* minimizer seeding */
    int wb; float wf;                /* adaptive band extra width */
    int zdrop, end_bonus;
    uint8_t ret_cigar:1, rev_cigar:1, out_msa:1, out_cons:1, out_gfa:1, out_fq:1, use_read_ids:1, amb_strand:1;
    uint8_t sub_aln:1, use_qv:1, disable_seeding:1, progressive_poa:1, put_gap_on_right:1, put_gap_at_end:1;
    char *incr_fn, *out_pog;
    int align_mode, gap_mode, max_n_cons, cons_algrm;
    double min_freq;
    int verbose;
    int batch_index;
} abpoa_para_t;

/* one graph node (abpoa.h:91-105) */
typedef struct {
    int node_id;
    int in_edge_n, in_edge_m, *in_id; int *in_edge_weight;
    int out_edge_n, out_edge_m, *out_id; int *out_edge_weight;
    int *read_weight, n_read, m_read, n_span_read;
    uint64_t **read_ids; int read_ids_n;
    int aligned_node_n, aligned_node_m, *aligned_node_id;
    uint8_t base;
} abpoa_node_t;

/* the DAG (abpoa.h:107-112) */
typedef struct {
    abpoa_node_t *node; int node_n, node_m, index_rank_m;
    int *index_to_node_id;
    int *node_id_to_index, *node_id_to_max_pos_left, *node_id_to_max_pos_right, *node_id_to_max_remain, *node_id_to_msa_rank;
    uint8_t is_topological_sorted:1, is_called_cons:1, is_set_msa_rank:1;
} abpoa_graph_t;

/* consensus / MSA results (abpoa.h:114-124) */
typedef struct {
    int n_cons, n_seq, msa_len;
    int *clu_n_seq;
    int **clu_read_ids;
    int *cons_len;
    int **cons_node_ids;
    uint8_t **cons_base;
    uint8_t **msa_base;
    int **cons_cov;
    int **cons_phred_score;
} abpoa_cons_t;

typedef struct { int l, m; char *s; } abpoa_str_t;           /* abpoa.h:126-128 */

typedef struct {
    int n_seq, m_seq;
    abpoa_str_t *seq, *name, *comment, *qual;
    uint8_t *is_rc;
} abpoa_seq_t;                                               /* abpoa.h:130-134 */

/* device-side DP arena; opaque to callers (abpoa.h:136) */
typedef struct abpoa_simd_matrix_t abpoa_simd_matrix_t;

typedef struct {
    abpoa_graph_t *abg;
    abpoa_seq_t *abs;
    abpoa_simd_matrix_t *abm;
    abpoa_cons_t *abc;
} abpoa_t;                                                   /* abpoa.h:138-143 */

/* ---- public API, 1:1 with the reference (abpoa.h:146-226) ---- */
abpoa_para_t *abpoa_init_para(void);
void abpoa_set_mat_from_file(abpoa_para_t *abpt, char *mat_fn);
void abpoa_post_set_para(abpoa_para_t *abpt);
void abpoa_free_para(abpoa_para_t *abpt);

abpoa_t *abpoa_init(void);
void abpoa_free(abpoa_t *ab);

int abpoa_msa(abpoa_t *ab, abpoa_para_t *abpt, int n_seqs, char **seq_names, int *seq_lens, uint8_t **seqs, int **qual_weights, FILE *out_fp);
void abpoa_clean_msa_cons(abpoa_t *ab);
int abpoa_msa1(abpoa_t *ab, abpoa_para_t *abpt, char *read_fn, FILE *out_fp);
void abpoa_reset(abpoa_t *ab, abpoa_para_t *abpt, int qlen);
abpoa_t *abpoa_restore_graph(abpoa_t *ab, abpoa_para_t *abpt);

int abpoa_align_sequence_to_graph(abpoa_t *ab, abpoa_para_t *abpt, uint8_t *query, int qlen, abpoa_res_t *res);
void abpoa_subgraph_nodes(abpoa_t *ab, abpoa_para_t *abpt, int inc_beg, int inc_end, int *exc_beg, int *exc_end);
int abpoa_align_sequence_to_subgraph(abpoa_t *ab, abpoa_para_t *abpt, int beg_node_id, int end_node_id, uint8_t *query, int qlen, abpoa_res_t *res);

int abpoa_add_graph_node(abpoa_graph_t *abg, uint8_t base);
int abpoa_add_graph_edge(abpoa_graph_t *abg, int from_id, int to_id, int check_edge, int w, uint8_t add_read_id, uint8_t add_read_weight, int read_id, int read_ids_n, int tot_read_n);
int abpoa_add_graph_alignment(abpoa_t *ab, abpoa_para_t *abpt, uint8_t *query, int *weight, int qlen, int *qpos_to_node_id, abpoa_res_t res, int read_id, int tot_read_n, int inc_both_ends);
int abpoa_add_subgraph_alignment(abpoa_t *ab, abpoa_para_t *abpt, int beg_node_id, int end_node_id, uint8_t *query, int *weight, int qlen, int *qpos_to_node_id, abpoa_res_t res, int read_id, int tot_read_n, int inc_both_ends);

void abpoa_BFS_set_node_index(abpoa_graph_t *abg, int src_id, int sink_id);
void abpoa_BFS_set_node_remain(abpoa_graph_t *abg, int src_id, int sink_id);
void abpoa_topological_sort(abpoa_graph_t *abg, abpoa_para_t *abpt);

void abpoa_generate_consensus(abpoa_t *ab, abpoa_para_t *abpt);
void abpoa_output_fx_consensus(abpoa_t *ab, abpoa_para_t *abpt, FILE *out_fp);
void abpoa_generate_rc_msa(abpoa_t *ab, abpoa_para_t *abpt);
void abpoa_output_rc_msa(abpoa_t *ab, abpoa_para_t *abpt, FILE *out_fp);
void abpoa_generate_gfa(abpoa_t *ab, abpoa_para_t *abpt, FILE *out_fp);
void abpoa_output(abpoa_t *ab, abpoa_para_t *abpt, FILE *out_fp);
void abpoa_dump_pog(abpoa_t *ab, abpoa_para_t *abpt);

/* ---- the drop-in aligner seam (abpoa_align_simd.h:11-12) ----
 * On a machine with an AMD GPU these run the HIP/CDNA4 core; with no GPU they
 * abort with a clear message (no silent CPU fallback). */
int simd_abpoa_align_sequence_to_graph(abpoa_t *ab, abpoa_para_t *abpt, uint8_t *query, int qlen, abpoa_res_t *res);
int simd_abpoa_align_sequence_to_subgraph(abpoa_t *ab, abpoa_para_t *abpt, int beg_node_id, int end_node_id, uint8_t *query, int qlen, abpoa_res_t *res);

/* ---- abpoa_amd extensions ---- */

/* Signature of an aligner implementation for the seam above. */
typedef int (*abpoa_amd_aligner_fn)(abpoa_t *ab, abpoa_para_t *abpt,
        int beg_node_id, int end_node_id, uint8_t *query, int qlen, abpoa_res_t *res);

/* TEST HOOK: replace the aligner implementation (used by tests to inject the
 * CPU oracle from oracle/liboracle.so on GPU-less machines). Prints a loud
 * notice; never called on the product path. Pass NULL to restore the GPU core. */
void abpoa_amd_set_test_aligner(abpoa_amd_aligner_fn fn);

/* Batched driver: run POA for many independent read-sets concurrently so the
 * GPU sees thousands of in-flight alignments. Processes sets[0..n_sets) where
 * each set is n_seqs sequences of seq_lens[s][i] bases (0..m-1 codes); writes
 * per-set consensus through the callback. Used by bench.py and the multi-GPU
 * sharding layer.
 *
 * With abpt->out_msa set (before abpoa_post_set_para, so that read ids are
 * tracked) the callback's abpoa_cons_t also carries the row-column MSA exactly
 * as abpoa_generate_rc_msa produces it for the same graph: msa_len columns and
 * msa_base rows of msa_len bytes each — n_seq read rows, followed by n_cons
 * consensus rows when abpt->out_cons is set — with gaps coded abpt->m. The
 * rows, like the rest of the result, are valid only during the callback. A
 * set with no graph has msa_len == 0. Without out_msa the result has
 * msa_len == 0 and msa_base == NULL, and no MSA work is done. */
typedef void (*abpoa_amd_cons_cb)(int set_idx, const abpoa_cons_t *cons, void *user);
int abpoa_amd_msa_batch(abpoa_para_t *abpt, int n_sets, const int *n_seqs,
        const int *const *seq_lens, const uint8_t *const *const *seqs,
        abpoa_amd_cons_cb cb, void *user, int n_host_threads);

/* Aggregate counters since last reset (for roofline reporting):
 * total DP cells computed by the device core and total device-kernel
 * nanoseconds measured with HIP events on the library's stream. */
void abpoa_amd_get_stats(uint64_t *dp_cells, uint64_t *kernel_ns, uint64_t *n_launches);
/* algorithmic HBM bytes of the plane streams (stored planes x score width x
 * cells: convex 3, affine 3, linear 1), summed per launch at the launch's
 * actual score width */
void abpoa_amd_get_stats2(uint64_t *alg_bytes);
void abpoa_amd_reset_stats(void);

/* Consensus stage of the batched driver. With the default configuration
 * (cons_algrm == ABPOA_HB, max_n_cons == 1) the device-resident driver
 * computes each set's consensus on the GPU after the last round and downloads
 * only the consensus (node ids, bases, coverage; phred is derived on the host
 * from the coverage). Every other configuration, a set with no graph, and any
 * set whose device job reports a non-OK status download the set's graph and
 * run abpoa_generate_consensus on host threads instead. Setting the
 * environment variable ABPOA_AMD_HOST_CONS (any value; read on every batch
 * call) forces that download path for all sets — outputs are identical, it
 * exists for A/B measurement.
 *
 * Counters are cumulative since the last reset:
 *   device_sets    sets whose consensus came from the device kernel
 *   host_sets      sets that took the graph-download path, for any reason
 *   fallback_sets  the subset of host_sets caused by a non-OK device status
 *   d2h_bytes      bytes the consensus stage copied device-to-host (either path)
 *   kernel_ns      consensus kernel time, measured with HIP events
 * Any pointer may be NULL. Builds without the GPU core report zeros. */
void abpoa_amd_get_cons_stats(uint64_t *device_sets, uint64_t *host_sets, uint64_t *fallback_sets,
                              uint64_t *d2h_bytes, uint64_t *kernel_ns);
void abpoa_amd_reset_cons_stats(void);

/* Row-column MSA stage of the batched driver; only sets of calls with
 * abpt->out_msa set are counted. A set takes the device path when it takes
 * the device consensus path (above), has a graph, and the environment
 * variable ABPOA_AMD_HOST_MSA is unset (any value; read on every batch call;
 * it sends every set to the graph-download path for consensus AND rows —
 * outputs are identical, it exists for A/B measurement). On the device path
 * two kernels build the matrix from the resident graph and only the matrix
 * is downloaded. A set is device for both stages or host for both: if either
 * device job reports a non-OK status that set alone falls back, and it is
 * counted as a fallback here and in the consensus counters.
 *
 * Counters are cumulative since the last reset:
 *   device_sets    sets whose rows came from the device kernels
 *   host_sets      sets whose rows came from abpoa_generate_rc_msa on a
 *                  downloaded graph, for any reason
 *   fallback_sets  the subset of host_sets caused by a non-OK device status
 *   d2h_bytes      bytes the rows cost device-to-host: per-set records plus
 *                  the matrix on the device path; the graph download on the
 *                  host path (that one download also serves the consensus and
 *                  is reported in the consensus counters too, as before)
 *   kernel_ns      MSA kernel time (both launches), measured with HIP events
 * Any pointer may be NULL. Builds without the GPU core report zeros. */
void abpoa_amd_get_msa_stats(uint64_t *device_sets, uint64_t *host_sets, uint64_t *fallback_sets,
                             uint64_t *d2h_bytes, uint64_t *kernel_ns);
void abpoa_amd_reset_msa_stats(void);

/* Multi-consensus (abpt->max_n_cons > 1) stage of the batched device-resident
 * driver. By default such calls download every set's graph for the host
 * clustering and consensus. With the environment variable
 * ABPOA_AMD_DEVICE_MULTICONS set (to anything not starting with '0'; read on
 * every batch call) the stage runs on the device for heaviest-bundle calls
 * with read-id tracking and an alphabet of at most 5 symbols, unless
 * ABPOA_AMD_HOST_CONS (or, with out_msa, ABPOA_AMD_HOST_MSA) is set: the read
 * rows of the row-column matrix are built there, a scan finds the candidate
 * heterozygous columns, only those columns come down for the host k-medoids
 * clustering, and one consensus pass per cluster runs on the device with
 * cluster-filtered edge weights. Outputs are identical on both paths. Sets
 * served there also count as device_sets of the consensus counters and, with
 * out_msa, of the MSA counters.
 *
 * Counters are cumulative since the last reset and count only calls with
 * max_n_cons > 1 made while the variable is set:
 *   device_sets       sets whose clusters and consensus came from the device stage
 *   host_sets         sets that took the graph-download path, for any reason
 *   fallback_sets     the subset of host_sets caused by a non-OK device status
 *   one_cluster_sets  device sets the clustering left in one cluster
 *   clusters          consensus sequences emitted for device sets
 *   cand_cols         candidate columns downloaded for device sets
 *   d2h_bytes         bytes the whole stage copied device-to-host
 *   kernel_ns         kernel time of the stage's launches (HIP events)
 * Any pointer may be NULL. Builds without the GPU core report zeros. */
void abpoa_amd_get_multicons_stats(uint64_t *device_sets, uint64_t *host_sets,
                                   uint64_t *fallback_sets, uint64_t *one_cluster_sets,
                                   uint64_t *clusters, uint64_t *cand_cols,
                                   uint64_t *d2h_bytes, uint64_t *kernel_ns);
void abpoa_amd_reset_multicons_stats(void);

/* Graph-fold stage of the batched device-resident driver. Each read of each
 * set is folded into the set's graph by one fold kernel job; the graph
 * mutation walk inside it runs across the job's 64 lanes (abamd_fold_par.inc).
 * The walk checks its own assumptions (one visit per node and per aligned
 * group, ids in range, bounded chains); a job in which a check fails leaves
 * the graph untouched and repeats the walk with the serial single-lane code,
 * so outputs never depend on the path. Setting the environment variable
 * ABPOA_AMD_SERIAL_FOLD (any value; read on every batch call) makes every job
 * use the single-lane walk — outputs are identical, it exists for A/B
 * measurement.
 *
 * Counters are cumulative since the last reset:
 *   parallel_folds  fold jobs whose walk ran on the lane-parallel path
 *   fallback_folds  fold jobs whose lane-parallel walk tripped a check and
 *                   was redone serially (expected: 0)
 *   serial_folds    fold jobs that ran the single-lane walk on request
 * Jobs that fold nothing (failed DP, pool overflow before the relaunch, empty
 * alignment) are not counted. Any pointer may be NULL. Builds without the GPU
 * core report zeros. */
void abpoa_amd_get_fold_stats(uint64_t *parallel_folds, uint64_t *fallback_folds,
                              uint64_t *serial_folds);
void abpoa_amd_reset_fold_stats(void);

/* Path counters of the batched drivers, for tests that must prove which
 * recovery path a run took. All are cumulative since the last reset:
 *   resident_calls     abpoa_amd_msa_batch calls served by the device-resident
 *                      driver
 *   hostfold_calls     calls served by the host-fold driver
 *   dp_retry_jobs      DP jobs of the resident driver whose arena reservation
 *                      overflowed and that were sent to the retry slot
 *   dp_retry_launches  launches on the retry slot; more than one per group of
 *                      failed jobs means a doubled reservation overflowed again
 *   pool_expands       graph-pool expansions (a set's slab doubled)
 *   big_chunks         chunks of items that exceeded the per-launch budget
 *   noop_folds         fold jobs that found an empty CIGAR on an existing
 *                      graph and left it untouched
 *   seam_retry_jobs    arena-overflow retries of the aligner seam (sequential
 *                      CLI and host-fold driver)
 *   launches_i16/_i32  DP launches of the resident driver by score width
 * Any pointer may be NULL. Builds without the GPU core count the calls and
 * report zeros for the rest. */
void abpoa_amd_get_batch_stats(uint64_t *resident_calls, uint64_t *hostfold_calls,
                               uint64_t *dp_retry_jobs, uint64_t *dp_retry_launches,
                               uint64_t *pool_expands, uint64_t *big_chunks,
                               uint64_t *noop_folds, uint64_t *seam_retry_jobs,
                               uint64_t *launches_i16, uint64_t *launches_i32);
void abpoa_amd_reset_batch_stats(void);

/* TEST HOOK: look at what the device-resident driver's fold kernel wrote,
 * fold by fold. With a probe installed the driver calls it once for every
 * fold job that settles — the first read's chain build, the folds of the
 * pipelined rounds, folds carried by a DP retry launch and folds relaunched
 * after a pool expansion alike — after synchronizing the job's stream and
 * downloading the set's state into host buffers the driver owns. The pointers
 * are valid only during the call. With no probe installed the cost is one
 * pointer test per settled fold.
 *
 * status is ABPOA_AMD_FOLD_PROBE_OK, or ABPOA_AMD_FOLD_PROBE_NOOP for a job
 * that found an empty CIGAR on an existing graph and left everything as it
 * was: then `out` carries the graph's counters only and every array pointer
 * and n_cigar is 0.
 *
 * Arrays hold their live counts: node arrays out.node_n entries, the in pools
 * out.edge_n_in, the out pools out.edge_n_out (rid_pool rid_n words per
 * out-edge, NULL when rid_n == 0), the aligned pool out.aln_n; i2n, n2i and
 * rem out.node_n entries (rem is unspecified when !use_remain: the kernel does
 * not write it); row_base, row_node_id and row_remain out.n_rows entries,
 * pre_off and out_off out.n_rows + 1, pre_idx out.n_pre, out_idx out.n_out.
 * cigar is the job's CIGAR in the forward order the fold consumed it; the
 * first read's chain build has none (n_cigar 0, cigar NULL).
 *
 * Threading: the driver runs every launch and every settle on the thread
 * that called abpoa_amd_msa_batch, so the probe is called on that thread,
 * from inside that call, one fold at a time. Install or remove it only while
 * no batch call is running. Builds without the GPU core accept and ignore
 * it. */
#define ABPOA_AMD_FOLD_PROBE_OK   0
#define ABPOA_AMD_FOLD_PROBE_NOOP 3
typedef struct {
    int set_idx, read_idx;
    int status;
    int walk;                    /* 0 single-lane on request, 1 lane-parallel,
                                    2 lane-parallel tripped a check, redone serially */
    int use_remain;              /* the job's: band or z-drop in use */
    int node_cap, edge_cap, aln_cap, rid_n;   /* the set's slab at this fold */
    struct {                     /* the record the kernel wrote for the job */
        int32_t status, node_n, edge_n_in, edge_n_out, aln_n, n_rows, n_pre, n_out, walk;
    } out;
    int n_cigar;
    const uint64_t *cigar;
    /* flat graph */
    const uint8_t *base;
    const int *n_read, *n_span_read;
    const int *in_head, *in_tail, *out_head, *out_tail, *aln_head;
    const int *in_to, *in_w, *in_next, *out_to, *out_w, *out_next;
    const uint64_t *rid_pool;
    const int *aln_id, *aln_next;
    /* derived: topological order and its inverse, max_remain */
    const int *i2n, *n2i, *rem;
    /* the next round's DP-row CSR */
    const uint8_t *row_base;
    const int *row_node_id, *pre_off, *out_off, *row_remain, *pre_idx, *out_idx;
} abpoa_amd_fold_probe_t;
typedef void (*abpoa_amd_fold_probe_fn)(const abpoa_amd_fold_probe_t *p, void *user);
void abpoa_amd_batch_set_fold_probe(abpoa_amd_fold_probe_fn fn, void *user);

#ifdef __cplusplus
}
#endif

#endif /* ABPOA_AMD_H */

/* Shared host<->device layout for the per-round device graph fold
 * (gpu_fold.hip :: abamd_fold_round_kernel).
 *
 * One job = one read set: consume the DP kernel's device-resident CIGAR,
 * mutate the set's device-resident flat graph (abamd_fold_core.inc — the
 * algorithm is CPU-twin-proven bit-equal to the pointer graph fold,
 * reference abpoa_graph.c:689-774), then re-derive topo index
 * (abpoa_graph.c:322-357), weight-sorted adjacency, remain BFS, n_span, and
 * materialize the next round's DP-row CSR (mirrors pack_job with the
 * identity row map). The batch driver (gpu_batch_resident.cpp) keeps every
 * graph resident in HBM across all rounds: no host fold, no per-round
 * repack, no per-round graph H2D.
 */
#ifndef ABAMD_GPU_FOLD_H
#define ABAMD_GPU_FOLD_H

#include <stdint.h>
#include "abamd_fold_core.h"   /* flat_graph_t */
#include "gpu_core.h"          /* abamd_gpu_res_t */

#ifdef __cplusplus
extern "C" {
#endif

enum {
    ABAMD_FOLD_OK = 0,
    ABAMD_FOLD_SKIPPED_DP = 1,   /* DP job failed (e.g. arena overflow): graph untouched */
    ABAMD_FOLD_POOL_OVERFLOW = 2,/* pre-checked pool exhaustion: graph untouched */
    ABAMD_FOLD_NOOP = 3          /* empty CIGAR on an existing graph: reference
                                    folds nothing (graph + derived state keep) */
};

/* per-set record the host reads back after each fold launch */
typedef struct {
    int32_t status;
    int32_t node_n, edge_n_in, edge_n_out, aln_n;
    int32_t n_rows, n_pre, n_out; /* DP-row CSR sizes for the next round */
    int32_t walk;                /* ABAMD_FOLD_WALK_*; set with status OK only */
} abamd_fold_out_t;

/* which mutation walk a fold job ran */
enum {
    ABAMD_FOLD_WALK_SERIAL = 0,  /* lane 0, on request (job.serial_fold) */
    ABAMD_FOLD_WALK_PARALLEL = 1,/* abamd_fold_par.inc across the wave */
    ABAMD_FOLD_WALK_FALLBACK = 2 /* parallel walk tripped a check: graph was
                                    untouched, lane 0 redid it serially */
};

/* one fold job; all pointers are device pointers into the set's slab */
typedef struct {
    flat_graph_t g;              /* counters = host mirror at launch time */
    uint64_t *cigar;             /* DP output, BACKTRACK order (kernel reverses) */
    const abamd_gpu_res_t *dp_res; /* NULL for the first read (chain build) */
    const uint8_t *seq;
    const int *weight;           /* shared all-ones buffer on this path */
    int seq_l;
    int read_id, add_read_id;
    int *index_to_node_id, *node_id_to_index, *max_remain, *scratch;
    /* DP-row CSR outputs for the next round's aligner launch */
    uint8_t *row_base;
    int *row_node_id, *pre_off, *out_off, *row_remain, *pre_idx, *out_idx;
    int use_remain;              /* abpt->wb >= 0 || abpt->zdrop > 0 */
    int m;                       /* alphabet size: bounds the aligned-pool pre-check */
    int serial_fold;             /* 1: lane-0 mutation walk (ABPOA_AMD_SERIAL_FOLD) */
    abamd_fold_out_t *out;
} abamd_fold_round_job_t;

/* launcher (gpu_fold.hip); stream is a hipStream_t */
void abamd_launch_fold_round(const abamd_fold_round_job_t *dev_jobs, int n_jobs, void *stream);

/* ---- device consensus (gpu_fold.hip :: abamd_cons_kernel) ----
 * One job = one read set's FINAL graph: single-cluster heaviest-bundle
 * consensus in four phases (abamd_cons_core.inc :: abamd_flat_cons_phased)
 * over the topological order the last fold left in i2n/n2i. The graph pools,
 * i2n and n2i are only read; the workspaces are slab regions that are dead
 * after the last fold. The host downloads `out` first, then cons_len entries
 * of cons_id/cons_base/cons_cov. */
typedef struct {
    int32_t status;              /* ABAMD_CONS_* (abamd_fold_core.h) */
    int32_t cons_len;
} abamd_cons_out_t;

typedef struct {
    flat_graph_t g;              /* device ptrs; counters = host mirror */
    const int *index_to_node_id, *node_id_to_index;
    int *max_w, *best, *score;   /* row space, >= n_rows ints each */
    int *cons_id;                /* also holds the row path before the gather */
    uint8_t *cons_base;
    int *cons_cov;
    abamd_cons_out_t *out;
} abamd_cons_job_t;

void abamd_launch_cons(const abamd_cons_job_t *dev_jobs, int n_jobs, void *stream);

/* ---- device row-column MSA (gpu_fold.hip :: abamd_msa_rank_kernel,
 * abamd_msa_place_kernel) ----
 * One job = one read set's FINAL graph, after abamd_cons_kernel on the same
 * stream. Launch A (rank) fills col[] and writes {status, msa_len}; the host
 * reads the records, lays the exact-size matrices out in one device buffer
 * pre-filled with the gap code, sets msa/msa_len in the jobs and runs launch
 * B (place), which writes the read rows and, when cons_len >= 0, one
 * consensus row from the ids and bases the consensus kernel left in the
 * slab, then overwrites `out->status`. The graph pools are only read; the
 * workspaces are slab regions that are dead once the consensus kernel has
 * run, and none of them is a consensus output. */
typedef struct {
    int32_t status;              /* ABAMD_MSA_* (abamd_fold_core.h) */
    int32_t msa_len;
} abamd_msa_out_t;

typedef struct {
    flat_graph_t g;              /* device ptrs; counters = host mirror */
    int *rank, *col;             /* node space, >= node_n ints each */
    int *in_deg, *stack;         /* node space, >= node_n ints each */
    const int *cons_id;          /* consensus kernel outputs (place only) */
    const uint8_t *cons_base;
    int cons_len;                /* < 0: no consensus row */
    int n_seq;
    uint8_t *msa;                /* (n_seq + (cons_len >= 0)) x msa_len, gap-filled */
    int msa_len;
    abamd_msa_out_t *out;
} abamd_msa_job_t;

void abamd_launch_msa_rank(const abamd_msa_job_t *dev_jobs, int n_jobs, void *stream);
void abamd_launch_msa_place(const abamd_msa_job_t *dev_jobs, int n_jobs, void *stream);

/* ---- device multi-consensus (gpu_fold.hip :: abamd_het_count_kernel,
 * abamd_het_gather_kernel, abamd_cons_clu_kernel, abamd_cons_row_kernel) ----
 * After abamd_msa_rank_kernel and abamd_msa_place_kernel (cons_len < 0) have
 * built a set's read rows: the het scan finds the candidate heterozygous
 * columns (launch 1 writes their indices to cand[] and {status, n_cand};
 * launch 2 gathers them into the row-major n_seq x n_cand matrix the host
 * clustering reads), then one abamd_cons_clu_kernel launch per cluster index
 * runs the heaviest-bundle pass with that cluster's read mask, and
 * abamd_cons_row_kernel places the cluster's consensus row. The graph pools,
 * i2n, n2i, col[] and the read rows are only read. */
typedef struct {
    int32_t status;              /* ABAMD_MSA_* */
    int32_t n_cand;
} abamd_het_out_t;

typedef struct {
    const uint8_t *msa;          /* n_seq x msa_len read rows */
    int n_seq, msa_len, m;
    int min_het, min_hom;        /* depth window (abamd_het_depth_bounds) */
    int *cand; int cand_cap;     /* candidate column indices, ascending */
    int n_cand;                  /* gather only: launch 1's count */
    uint8_t *out;                /* gather only: n_seq x n_cand */
    abamd_het_out_t *rec;
} abamd_het_job_t;

void abamd_launch_het_count(const abamd_het_job_t *dev_jobs, int n_jobs, void *stream);
void abamd_launch_het_gather(const abamd_het_job_t *dev_jobs, int n_jobs, void *stream);

typedef struct {
    abamd_cons_job_t c;          /* as for abamd_cons_kernel */
    const uint64_t *mask;        /* the cluster's read ids, c.g.rid_n words */
} abamd_cons_clu_job_t;

void abamd_launch_cons_clu(const abamd_cons_clu_job_t *dev_jobs, int n_jobs, void *stream);

typedef struct {
    int node_n;
    const int *col;              /* abamd_msa_rank_kernel's columns */
    const int *cons_id;          /* consensus kernel outputs */
    const uint8_t *cons_base;
    int cons_len;
    uint8_t *row; int msa_len;   /* the gap-filled consensus row */
    abamd_msa_out_t *out;        /* status only; msa_len is left alone */
} abamd_cons_row_job_t;

void abamd_launch_cons_row(const abamd_cons_row_job_t *dev_jobs, int n_jobs, void *stream);

#ifdef __cplusplus
}
#endif

#endif

/* Flat-array graph fold core (see abamd_fold_core.c). Device-layout graph
 * mutation, bit-exact with the pointer-based abamd_graph.c fold. */
#ifndef ABAMD_FOLD_CORE_H
#define ABAMD_FOLD_CORE_H

#include <stdint.h>

typedef struct flat_graph_t {
    int node_n, node_cap;
    uint8_t *base;               /* [node_cap] */
    int *n_read, *n_span_read;   /* [node_cap] */
    /* append-only per-direction edge pools; per-node head/tail chains keep
     * the pointer graph's append order */
    int edge_n_in, edge_n_out, edge_cap;
    int *in_head, *in_tail, *out_head, *out_tail;   /* [node_cap] */
    int *in_to, *in_w, *in_next;                    /* [edge_cap] */
    int *out_to, *out_w, *out_next;                 /* [edge_cap] */
    uint64_t *rid_pool; int rid_n;  /* per-OUT-edge read-id bitsets (words) */
    /* aligned (mismatch-column) groups as linked lists */
    int aln_n, aln_cap;
    int *aln_head;                                  /* [node_cap] */
    int *aln_id, *aln_next;                         /* [aln_cap] */
} flat_graph_t;

/* phased flat consensus (abamd_cons_core.inc): per-job status and the row
 * count staged per step of the reverse sweep (= the device wave width) */
enum {
    ABAMD_CONS_OK = 0,
    ABAMD_CONS_BAD_GRAPH = 1     /* no SRC->SINK walk through the chosen edges:
                                    only a corrupt graph / topo order gives it */
};
#define ABAMD_CONS_CHUNK 64

/* phased flat row-column MSA (abamd_msa_core.inc): per-job status */
enum {
    ABAMD_MSA_OK = 0,
    ABAMD_MSA_BAD_GRAPH = 1      /* an index out of its pool, a walk past its
                                    bound, a read id >= n_seq or a column
                                    outside the matrix: only a corrupt graph */
};

/* het scan (abamd_msa_core.inc): largest alphabet whose m + 1 depth counters
 * it keeps in scalars, and the ints of its shared staging area (status word,
 * spare, one flag per lane of a 64-lane group) */
#define ABAMD_HET_MAX_M 5
#define ABAMD_HET_STAGE (2 + 64)

/* lane-parallel mutation walk (abamd_fold_par.inc): scratch and per-call
 * state. The six arrays hold `cap` ints each, `part` holds part_cap >=
 * ABAMD_PAR_PARTS * n_lanes ints; none of them overlaps another or the graph. */
#define ABAMD_PAR_PHASES 6
#define ABAMD_PAR_PARTS 6
/* part[k * n_lanes + lane]: violation flag, query bases consumed, new nodes,
 * aligned-pool entries, last existing path node (-1: none), new edges */
enum { FLAT_PAR_BAD = 0, FLAT_PAR_C, FLAT_PAR_NN, FLAT_PAR_NA, FLAT_PAR_LAST, FLAT_PAR_NE };
typedef struct flat_par_ws_t {
    int *owner;                  /* node id -> claiming op */
    int *path, *nsp;             /* query pos -> path node, inherited n_span_read */
    int *opres;                  /* op -> existing path node, or -1: creates one */
    int *e_in, *e_out;           /* path edge -> existing edge id, or -1 */
    int cap;
    int *part; int part_cap;     /* per-lane partial sums and flags */
} flat_par_ws_t;
typedef struct flat_par_t {
    flat_graph_t *fg;
    int beg, end;
    const uint8_t *seq; const int *weight; int seq_l;
    int *qpos;
    int n_cigar; const uint64_t *cig;
    int read_id, add_read_id, inc_both_ends;
    int node_n0, ein0, eout0, aln0;   /* counters before the walk */
    int nn_tot, na_tot, ne_tot;       /* new nodes, aligned entries, edges */
    flat_par_ws_t ws;
    int mode, ok;
} flat_par_t;

/* Device translation units (gpu_fold.hip) include this header for the
 * flat_graph_t layout only: the function bodies there are __device__ builds
 * of abamd_fold_core.inc, and host declarations of the same names would
 * clash with them. */
#ifndef ABAMD_FC_NO_HOST_DECLS
#ifdef __cplusplus
extern "C" {
#endif

void abamd_flat_init(flat_graph_t *fg, int node_cap, int edge_cap, int aln_cap, int rid_n);
void abamd_flat_free(flat_graph_t *fg);
void abamd_flat_sort_adjacency(flat_graph_t *fg);
void abamd_flat_topo_index(const flat_graph_t *fg, int *index_to_node_id,
                           int *node_id_to_index, int *scratch);
void abamd_flat_remain(const flat_graph_t *fg, int *max_remain, int *scratch);
void abamd_flat_update_n_span(flat_graph_t *fg, const int *index_to_node_id,
                              const int *node_id_to_index, int inc_both_ends);
void abamd_flat_msa_rank(const flat_graph_t *fg, int *msa_rank_out, int *scratch);
int abamd_flat_build_rows(const flat_graph_t *fg, const int *index_to_node_id,
                          const int *node_id_to_index, const int *max_remain,
                          int use_remain, uint8_t *row_base, int *row_node_id,
                          int *pre_off, int *out_off, int *remain,
                          int *pre_idx, int *out_idx);
void abamd_flat_apply_alignment(flat_graph_t *fg, int beg_node_id, int end_node_id,
                                const uint8_t *seq, const int *weight, int seq_l,
                                int *qpos_to_node_id, int n_cigar, const abpoa_cigar_t *cig,
                                int read_id, int add_read_id, int inc_both_ends);

/* the same walk in lane-parallel phases (abamd_fold_par.inc). Returns 1 when
 * applied, 0 when a guard tripped: the graph is untouched and the caller runs
 * abamd_flat_apply_alignment. Host use: lane 0 of 1, or init + a loop over
 * the lanes inside each of the ABAMD_PAR_PHASES phases to emulate a wave. */
int abamd_flat_apply_par(flat_graph_t *fg, int beg_node_id, int end_node_id,
                         const uint8_t *seq, const int *weight, int seq_l,
                         int *qpos_to_node_id, int n_cigar, const abpoa_cigar_t *cig,
                         int read_id, int add_read_id, int inc_both_ends,
                         const flat_par_ws_t *ws, int lane, int n_lanes);
void abamd_flat_par_init(flat_par_t *cx, flat_graph_t *fg, int beg_node_id, int end_node_id,
                         const uint8_t *seq, const int *weight, int seq_l,
                         int *qpos_to_node_id, int n_cigar, const abpoa_cigar_t *cig,
                         int read_id, int add_read_id, int inc_both_ends,
                         const flat_par_ws_t *ws, int n_lanes);
void abamd_flat_par_phase(flat_par_t *cx, int phase, int lane, int n_lanes);

/* single-cluster heaviest-bundle consensus over the flat layout
 * (abamd_cons_core.inc); returns cons_len */
int abamd_flat_hb_consensus(const flat_graph_t *fg, int n_seq,
                            int *scratch, int *score, int *max_out,
                            int *cons_id, uint8_t *cons_base,
                            int *cons_cov, int *cons_phred);

/* the same consensus in four phases over the fold's topological order
 * (rows 0..n2i[SINK]); host build of the device kernel's body — call with
 * lane 0 of 1. Workspaces: max_w/best/score/path n2i[SINK]+1 ints, stage
 * 3*ABAMD_CONS_CHUNK ints; cons_id may alias path. Returns ABAMD_CONS_*. */
int abamd_flat_cons_phased(const flat_graph_t *fg, const int *i2n, const int *n2i,
                           int *max_w, int *best, int *score, int *path,
                           int *cons_id, uint8_t *cons_base, int *cons_cov,
                           int *stage, int *cons_len_out, int lane, int n_lanes);

/* row-column MSA in two stages over the flat graph (abamd_msa_core.inc);
 * host build of the device kernels' bodies — call with lane 0 of 1.
 * Stage 1: rank/col/in_deg/stack hold node_n ints each, stage 2 ints; yields
 * msa_len and each node's column in col[]. Stage 2: msa is a row-major
 * (n_seq + (cons_len >= 0)) x msa_len matrix pre-filled with the gap code.
 * Both return ABAMD_MSA_*. */
int abamd_flat_msa_rank_cols(const flat_graph_t *fg, int *rank, int *col,
                             int *in_deg, int *stack, int *stage,
                             int *msa_len_out, int lane, int n_lanes);
int abamd_flat_msa_place(const flat_graph_t *fg, const int *col, int n_seq,
                         int msa_len, uint8_t *msa, const int *cons_id,
                         const uint8_t *cons_base, int cons_len,
                         int *stage, int lane, int n_lanes);

/* one heaviest-bundle pass with cluster-filtered edge weights (multi-consensus,
 * n_clu >= 2): abamd_flat_cons_phased plus the cluster's read-id mask of
 * fg->rid_n words; coverage is the cluster's reads over the node's out-edges */
int abamd_flat_cons_phased_clu(const flat_graph_t *fg, const uint64_t *mask,
                               const int *i2n, const int *n2i,
                               int *max_w, int *best, int *score, int *path,
                               int *cons_id, uint8_t *cons_base, int *cons_cov,
                               int *stage, int *cons_len_out, int lane, int n_lanes);

/* one consensus row of the row-column MSA as a stage of its own: `row` holds
 * msa_len bytes pre-filled with the gap code; stage 2 ints */
int abamd_flat_msa_place_cons_row(int node_n, const int *col, int msa_len, uint8_t *row,
                                  const int *cons_id, const uint8_t *cons_base, int cons_len,
                                  int *stage, int lane, int n_lanes);

/* het scan over the read rows (abamd_msa_core.inc). Count: the candidate
 * columns' indices, ascending, into cand[cand_cap]; stage ABAMD_HET_STAGE
 * ints. Gather: those columns as a row-major n_seq x n_cand matrix; stage 2
 * ints. Both return ABAMD_MSA_*. */
int abamd_flat_het_count(const uint8_t *msa, int n_seq, int msa_len, int m,
                         int min_het, int min_hom, int *cand, int cand_cap,
                         int *stage, int *n_cand_out, int lane, int n_lanes);
int abamd_flat_het_gather(const uint8_t *msa, int n_seq, int msa_len, const int *cand,
                          int n_cand, uint8_t *out, int *stage, int lane, int n_lanes);

#ifdef ABPOA_AMD_H
/* the depth window of a candidate het column for n_seq reads (abamd_cons.c) */
void abamd_het_depth_bounds(int n_seq, const abpoa_para_t *abpt, int *min_het, int *min_hom);
/* read clustering from an n_seq x msa_l matrix that holds all columns or the
 * candidate het columns only (abamd_cons.c): returns n_clu; for n_clu >= 2
 * *clu_read_ids gets n_clu separately allocated bitsets of (n_seq-1)/64+1 words */
int abamd_read_clu_from_msa(uint8_t **msa, int msa_l, int n_seq, abpoa_para_t *abpt,
                            uint64_t ***clu_read_ids);
/* the n_clu >= 2 result from per-cluster consensus paths (abamd_cons.c);
 * masks holds n_clu * ((n_seq-1)/64+1) words. `abc` must be cleared. */
void abamd_cons_from_paths(abpoa_cons_t *abc, int n_seq, int n_clu, const uint64_t *masks,
                           const int *cons_len, const int *const *ids,
                           const uint8_t *const *bases, const int *const *cov);
/* Build the single-cluster abpoa_cons_t the heaviest-bundle pass produces
 * from a consensus path (abamd_cons.c): phred from coverage on the host,
 * n_cons = 1, every read in cluster 0. `abc` must be cleared. */
void abamd_cons_from_path(abpoa_cons_t *abc, int n_seq, int cons_len, const int *ids,
                          const uint8_t *bases, const int *cov);
/* Attach a row-column MSA to a result built by abamd_cons_from_path
 * (abamd_cons.c): `rows` is a row-major n_rows x msa_len matrix with
 * n_rows = n_seq, or n_seq + n_cons with the consensus rows last. msa_base
 * gets n_seq + n_cons separately allocated rows, the layout
 * abpoa_generate_rc_msa produces and abamd_cons_clear frees; rows beyond
 * n_rows hold the gap code. */
void abamd_cons_attach_msa(abpoa_cons_t *abc, int n_rows, int msa_len, const uint8_t *rows,
                           int gap);
/* free an abpoa_cons_t's arrays, MSA rows included, and zero it (abamd_graph.c) */
void abamd_cons_clear(abpoa_cons_t *abc);
/* Rebuild a pointer graph from a (host copy of a) flat graph and topo-sort
 * it — the device-resident batch driver's hand-off to the host consensus
 * path (abamd_graph.c). `ab` must be fresh. All node arrays are carved from
 * ONE returned slab; call abamd_graph_arena_release(ab, slab) before
 * abpoa_free(ab). */
void *abamd_graph_from_flat(abpoa_t *ab, const flat_graph_t *fg, abpoa_para_t *abpt, int read_ids_n,
                            const int *i2n, const int *n2i, const int *remain);
void abamd_graph_arena_release(abpoa_t *ab, void *slab);
#endif

#ifdef __cplusplus
}
#endif
#endif /* ABAMD_FC_NO_HOST_DECLS */

#endif

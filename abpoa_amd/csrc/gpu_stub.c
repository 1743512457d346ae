/* Link stub used ONLY by the CPU-side test build (abpoa_amd_cputest): the
 * product GPU core is not linked, so any attempt to use the product aligner
 * without an explicitly injected test oracle aborts loudly. */
#include "abpoa_amd.h"
#include "abamd_util.h"

int abamd_gpu_align_sequence_to_subgraph(abpoa_t *ab, abpoa_para_t *abpt,
        int beg_node_id, int end_node_id, uint8_t *query, int qlen, abpoa_res_t *res) {
    (void)ab; (void)abpt; (void)beg_node_id; (void)end_node_id; (void)query; (void)qlen; (void)res;
    abamd_fatal("abpoa_amd", "this is the CPU-only TEST build: no GPU aligner is linked. "
                "Inject the oracle via ABPOA_AMD_TEST_ALIGNER_SO, or use the real abpoa_amd build.");
    return -1;
}

void abpoa_amd_get_stats(uint64_t *dp_cells, uint64_t *kernel_ns, uint64_t *n_launches) {
    if (dp_cells) *dp_cells = 0;
    if (kernel_ns) *kernel_ns = 0;
    if (n_launches) *n_launches = 0;
}
void abpoa_amd_reset_stats(void) {}

typedef struct {
    abpoa_t *ab; abpoa_para_t *abpt;
    int beg_node_id, end_node_id;
    uint8_t *query; int qlen; abpoa_res_t *res;
    int64_t est_cells_hint; int64_t *cells_out;
} abamd_batch_job_t;

int abamd_gpu_align_batch(abamd_batch_job_t *batch, int n_jobs) {
    /* CPU test build: route each job through the dispatching seam so an
     * injected test oracle serves batched runs too. */
    int i;
    for (i = 0; i < n_jobs; ++i)
        simd_abpoa_align_sequence_to_subgraph(batch[i].ab, batch[i].abpt,
            batch[i].beg_node_id, batch[i].end_node_id, batch[i].query, batch[i].qlen, batch[i].res);
    return 0;
}

void abpoa_amd_get_stats2(uint64_t *alg_bytes) { if (alg_bytes) *alg_bytes = 0; }

/* no device consensus in the CPU test build: the counters stay zero */
void abpoa_amd_get_cons_stats(uint64_t *device_sets, uint64_t *host_sets, uint64_t *fallback_sets,
                              uint64_t *d2h_bytes, uint64_t *kernel_ns) {
    if (device_sets) *device_sets = 0;
    if (host_sets) *host_sets = 0;
    if (fallback_sets) *fallback_sets = 0;
    if (d2h_bytes) *d2h_bytes = 0;
    if (kernel_ns) *kernel_ns = 0;
}
void abpoa_amd_reset_cons_stats(void) {}
/* nor a device MSA: the host-fold driver builds the rows on host threads */
void abpoa_amd_get_msa_stats(uint64_t *device_sets, uint64_t *host_sets, uint64_t *fallback_sets,
                             uint64_t *d2h_bytes, uint64_t *kernel_ns) {
    if (device_sets) *device_sets = 0;
    if (host_sets) *host_sets = 0;
    if (fallback_sets) *fallback_sets = 0;
    if (d2h_bytes) *d2h_bytes = 0;
    if (kernel_ns) *kernel_ns = 0;
}
void abpoa_amd_reset_msa_stats(void) {}
/* nor a device multi-consensus */
void abpoa_amd_get_multicons_stats(uint64_t *device_sets, uint64_t *host_sets,
                                   uint64_t *fallback_sets, uint64_t *one_cluster_sets,
                                   uint64_t *clusters, uint64_t *cand_cols,
                                   uint64_t *d2h_bytes, uint64_t *kernel_ns) {
    if (device_sets) *device_sets = 0;
    if (host_sets) *host_sets = 0;
    if (fallback_sets) *fallback_sets = 0;
    if (one_cluster_sets) *one_cluster_sets = 0;
    if (clusters) *clusters = 0;
    if (cand_cols) *cand_cols = 0;
    if (d2h_bytes) *d2h_bytes = 0;
    if (kernel_ns) *kernel_ns = 0;
}
void abpoa_amd_reset_multicons_stats(void) {}
/* nor a device fold */
void abpoa_amd_get_fold_stats(uint64_t *parallel_folds, uint64_t *fallback_folds,
                              uint64_t *serial_folds) {
    if (parallel_folds) *parallel_folds = 0;
    if (fallback_folds) *fallback_folds = 0;
    if (serial_folds) *serial_folds = 0;
}
void abpoa_amd_reset_fold_stats(void) {}
/* the call counters live in abamd_batch.c; nothing else exists here */
extern uint64_t abamd_batch_calls[2];
void abpoa_amd_get_batch_stats(uint64_t *resident_calls, uint64_t *hostfold_calls,
                               uint64_t *dp_retry_jobs, uint64_t *dp_retry_launches,
                               uint64_t *pool_expands, uint64_t *big_chunks,
                               uint64_t *noop_folds, uint64_t *seam_retry_jobs,
                               uint64_t *launches_i16, uint64_t *launches_i32) {
    if (resident_calls) *resident_calls = abamd_batch_calls[0];
    if (hostfold_calls) *hostfold_calls = abamd_batch_calls[1];
    if (dp_retry_jobs) *dp_retry_jobs = 0;
    if (dp_retry_launches) *dp_retry_launches = 0;
    if (pool_expands) *pool_expands = 0;
    if (big_chunks) *big_chunks = 0;
    if (noop_folds) *noop_folds = 0;
    if (seam_retry_jobs) *seam_retry_jobs = 0;
    if (launches_i16) *launches_i16 = 0;
    if (launches_i32) *launches_i32 = 0;
}
void abpoa_amd_reset_batch_stats(void) { abamd_batch_calls[0] = abamd_batch_calls[1] = 0; }
/* no device fold to look at */
void abpoa_amd_batch_set_fold_probe(abpoa_amd_fold_probe_fn fn, void *user) { (void)fn; (void)user; }
void abamd_timing_report(const char *tag) { (void)tag; }

static abamd_batch_job_t *stub_slot_batch[8];
static int stub_slot_n[8];
int abamd_gpu_batch_prepare(abamd_batch_job_t *batch, int n_jobs, int slot) {
    stub_slot_batch[slot] = batch; stub_slot_n[slot] = n_jobs; return 0;
}
int abamd_gpu_batch_launch(int slot) {
    return abamd_gpu_align_batch(stub_slot_batch[slot], stub_slot_n[slot]);
}
int abamd_gpu_batch_finish_slot(int slot) { (void)slot; return 0; }

int abamd_gpu_align_batch_slot(abamd_batch_job_t *batch, int n_jobs, int slot) {
    (void)slot; return abamd_gpu_align_batch(batch, n_jobs);
}

int64_t abamd_gpu_free_mem(void) { return 0; }
void abamd_gpu_set_arena_cap(uint64_t bytes) { (void)bytes; }

/* device-resident batch driver: GPU build only — the CPU test build always
 * takes the host-fold driver */
int abamd_batch_resident_supported(const abpoa_para_t *abpt) { (void)abpt; return 0; }
int abpoa_amd_msa_batch_resident(abpoa_para_t *abpt, int n_sets, const int *n_seqs,
                                 const int *const *seq_lens, const uint8_t *const *const *seqs,
                                 abpoa_amd_cons_cb cb, void *user, int n_host_threads) {
    (void)abpt; (void)n_sets; (void)n_seqs; (void)seq_lens; (void)seqs;
    (void)cb; (void)user; (void)n_host_threads;
    abamd_fatal("abpoa_amd", "device-resident batch driver is not in the CPU test build");
    return -1;
}

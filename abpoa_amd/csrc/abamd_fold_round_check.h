/* Per-round check of the production fold kernel's outputs
 * (abamd_fold_round_check.c): a host flat-graph twin per read set, advanced
 * by the serial abamd_flat_* passes on every fold-probe call
 * (abpoa_amd_batch_set_fold_probe) and compared with what the probe hands
 * over. Linked by abpoa_amd_batchgpu (--fold-check, the device under test)
 * and by abpoa_amd_foldroundtwin (the comparison's own CPU self-test). */
#ifndef ABAMD_FOLD_ROUND_CHECK_H
#define ABAMD_FOLD_ROUND_CHECK_H

#include <stdio.h>
#include "abpoa_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct abamd_frc_t abamd_frc_t;

/* the read sets exactly as abpoa_amd_msa_batch gets them; they must outlive
 * the checker. abpt supplies m and use_read_ids. */
abamd_frc_t *abamd_frc_new(const abpoa_para_t *abpt, int n_sets, const int *n_seqs,
                           const int *const *seq_lens, const uint8_t *const *const *seqs);
/* one probe call. Returns 0 when everything agrees. On the first difference
 * prints one line to `err`,
 *   fold-check MISMATCH set S read R field NAME index I: device X twin Y
 * returns 1, and ignores every later call (the twin of that set is no longer
 * in step). */
int abamd_frc_check(abamd_frc_t *c, const abpoa_amd_fold_probe_t *p, FILE *err);
int abamd_frc_failed(const abamd_frc_t *c);
/* one line:
 *   [fold-check] folds=N noop=N parallel=N fallback=N serial=N max_in_deg=N
 *   max_out_deg=N max_n_rows=N min_n_rows=N caps_grew=0|1 rows_by_set=a,b,...
 * folds counts the compared (status OK) calls, noop the no-op ones;
 * rows_by_set is each set's n_rows after its last fold (0: never folded). */
void abamd_frc_summary(const abamd_frc_t *c, FILE *f);
void abamd_frc_free(abamd_frc_t *c);

#ifdef __cplusplus
}
#endif

#endif

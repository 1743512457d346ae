/* The command line's option loop, shared by the CLI (abamd_cli.c) and the
 * batch harness (abamd_batch_test.c) so that both spell every option alike and
 * give it the same effect on abpt. Option surface mirrors the reference CLI
 * (abpoa.c:170-250). */
#include <getopt.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"

#define ABPOA_AMD_VERSION "0.1.0-r1"

/* Parses argv into abpt (before abpoa_post_set_para) and leaves optind at the
 * first operand. in_list receives -l. harness_stats, when not NULL, takes -S
 * for the caller (the batch harness's stats line; seeding has no meaning in
 * the batched driver); when NULL -S switches seeding on as in the CLI.
 * Returns 0 to go on, 1 for a usage error, -1 when the call is complete
 * (-v). */
int abamd_cli_parse_opts(int argc, char **argv, abpoa_para_t *abpt, int *in_list, int *harness_stats) {
    int c, m; char *s;
    while ((c = getopt(argc, argv, "m:M:X:t:O:E:b:f:z:e:GLRJQSk:w:n:i:clpso:r:g:a:d:q:hvV:")) >= 0) {
        switch (c) {
            case 'm': m = atoi(optarg);
                      if (m != ABPOA_GLOBAL_MODE && m != ABPOA_EXTEND_MODE && m != ABPOA_LOCAL_MODE) {
                          fprintf(stderr, "Unknown alignment mode: %d.\n", m); return 1;
                      } abpt->align_mode = m; break;
            case 'M': abpt->match = atoi(optarg); break;
            case 'X': abpt->mismatch = atoi(optarg); break;
            case 't': abpt->use_score_matrix = 1; abpt->mat_fn = strdup(optarg); break;
            case 'O': abpt->gap_open1 = (int)strtol(optarg, &s, 10);
                      abpt->gap_open2 = (*s == ',') ? (int)strtol(s + 1, &s, 10) : 0; break;
            case 'E': abpt->gap_ext1 = (int)strtol(optarg, &s, 10);
                      abpt->gap_ext2 = (*s == ',') ? (int)strtol(s + 1, &s, 10) : 0; break;
            case 'G': abpt->inc_path_score = 1; break;
            case 'L': abpt->sort_input_seq = 1; break;
            case 'R': abpt->put_gap_on_right = 1; break;
            case 'J': abpt->put_gap_at_end = 1; break;
            case 'b': abpt->wb = atoi(optarg); break;
            case 'f': abpt->wf = (float)atof(optarg); break;
            case 'z': abpt->zdrop = atoi(optarg); break;
            case 'e': abpt->end_bonus = atoi(optarg); break;
            case 'Q': abpt->use_qv = 1; break;
            case 'S': if (harness_stats) *harness_stats = 1; else abpt->disable_seeding = 0; break;
            case 'k': abpt->k = atoi(optarg); break;
            case 'w': abpt->w = atoi(optarg); break;
            case 'n': abpt->min_w = atoi(optarg); break;
            case 'c': abpt->m = 27;
                      abpt->mat = (int*)abamd_realloc(abpt->mat, (size_t)abpt->m * abpt->m * sizeof(int)); break;
            case 'i': abpt->incr_fn = strdup(optarg); break;
            case 'l': if (in_list) *in_list = 1; break;
            case 'p': abpt->progressive_poa = 1; break;
            case 's': abpt->amb_strand = 1; break;
            case 'o': if (strcmp(optarg, "-") != 0) {
                          if (freopen(optarg, "wb", stdout) == NULL)
                              abamd_fatal("abpoa_amd", "failed to open output file %s", optarg);
                      } break;
            case 'r': if (atoi(optarg) == ABPOA_OUT_CONS) abpt->out_cons = 1, abpt->out_msa = 0;
                      else if (atoi(optarg) == ABPOA_OUT_MSA) abpt->out_cons = 0, abpt->out_msa = 1;
                      else if (atoi(optarg) == ABPOA_OUT_CONS_MSA) abpt->out_cons = abpt->out_msa = 1;
                      else if (atoi(optarg) == ABPOA_OUT_GFA) abpt->out_cons = 0, abpt->out_gfa = 1;
                      else if (atoi(optarg) == ABPOA_OUT_CONS_GFA) abpt->out_cons = 1, abpt->out_gfa = 1;
                      else if (atoi(optarg) == ABPOA_OUT_CONS_FQ) abpt->out_cons = 1, abpt->out_fq = 1;
                      else fprintf(stderr, "Error: unknown output result mode: %s.\n", optarg);
                      break;
            case 'g': abpt->out_pog = strdup(optarg); break;
            case 'a': abpt->cons_algrm = atoi(optarg); break;
            case 'd': abpt->max_n_cons = atoi(optarg);
                      if (abpt->max_n_cons < 1 || abpt->max_n_cons > 10) {
                          fprintf(stderr, "Error: max number of consensus sequences should be 1~10.\n");
                          return 1;
                      } break;
            case 'q': abpt->min_freq = atof(optarg); break;
            case 'h': return 1;
            case 'V': abpt->verbose = atoi(optarg); break;
            case 'v': printf("%s\n", ABPOA_AMD_VERSION); return -1;
            default: return 1;
        }
    }
    return 0;
}

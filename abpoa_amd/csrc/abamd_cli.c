/* abpoa_amd command-line interface.
 * Option surface mirrors the reference CLI (abpoa.c:170-250) so parity tests
 * can drive both binaries with identical argv; stdout framing is identical,
 * diagnostics go to stderr. */
#include <getopt.h>
#include <string.h>
#include "abpoa_amd.h"
#include "abamd_util.h"

static int usage(void) {
    fprintf(stderr, "Usage: abpoa_amd [options] <in.fa/fq> > cons.fa\n");
    fprintf(stderr, "  MI355X-native abPOA-compatible POA. Options match the reference abpoa CLI;\n");
    fprintf(stderr, "  see the reference usage for details. Unsupported in this build: -S -p -i -d>=2 -s -g.\n");
    return 1;
}

static int abpoa_amd_main(char *file_fn, int is_list, abpoa_para_t *abpt) {
    double t0 = abamd_realtime();
    abpoa_t *ab = abpoa_init();
    if (is_list) {
        FILE *list_fp = fopen(file_fn, "r"); char read_fn[1024];
        if (!list_fp) abamd_fatal("abpoa_amd", "cannot open list file '%s'", file_fn);
        int batch_index = 1;
        while (fgets(read_fn, sizeof(read_fn), list_fp)) {
            size_t l = strlen(read_fn);
            if (l && read_fn[l-1] == '\n') read_fn[l-1] = 0;
            abpt->batch_index = batch_index;
            abpoa_msa1(ab, abpt, read_fn, stdout);
            batch_index++;
        }
        fclose(list_fp);
    } else abpoa_msa1(ab, abpt, file_fn, stdout);
    abpoa_free(ab);
    fprintf(stderr, "[abpoa_amd_main] Real time: %.3f sec; CPU: %.3f sec; Peak RSS: %.3f GB.\n",
            abamd_realtime() - t0, abamd_cputime(), abamd_peakrss() / 1024.0 / 1024.0);
    return 0;
}

int abamd_cli_parse_opts(int argc, char **argv, abpoa_para_t *abpt, int *in_list, int *harness_stats);
void abamd_timing_report(const char *tag);

int main(int argc, char **argv) {
    int c, in_list = 0;
    abpoa_para_t *abpt = abpoa_init_para();
    c = abamd_cli_parse_opts(argc, argv, abpt, &in_list, NULL);
    if (c < 0) { abpoa_free_para(abpt); return 0; }
    if (c > 0) return usage();
    if (argc - optind != 1) return usage();
    abpoa_post_set_para(abpt);
    fprintf(stderr, "[abpoa_amd] CMD:");
    for (c = 0; c < argc; ++c) fprintf(stderr, " %s", argv[c]);
    fprintf(stderr, "\n");
    abpoa_amd_main(argv[optind], in_list, abpt);
    abamd_timing_report("cli"); /* under ABPOA_AMD_TIMING: the seam's phase times and retry count */
    abpoa_free_para(abpt);
    return 0;
}

// eco -- flag-compatible replacement of cli/eco.cpp (ECO, the sampled-softmax
// choice rule: per sample a field-0 source and five lists of two positives and
// negative_samples negatives; src/model/ECO.cpp:64-128, src/proNet.cpp:2221-2341).
// Extra flags: -device, -mode atomic|hybrid|serial, -seed, -format cpp|go,
// -stop_after <n> (run only the first n samples of the sample_times x 10^6
// schedule).  One GPU only.
#include "cli_common.h"

int main(int argc, char** argv) {
    int i;
    if (argc == 1) {
        printf("[smore-mi355x] ECO\n\nOptions Description:\n");
        printf("\t-train <string>\n\t-save <string>\n\t-field <string>\n\t-dimensions <int> (64)\n");
        printf("\t-negative_samples <int> (5)\n\t-sample_times <int> (10, x10^6)\n\t-alpha <float> (0.025)\n");
        printf("\t-reg <float> (0.01)\n\t-threads <int>\n");
        printf("\t-device <int> -mode atomic|hybrid|serial -seed <int> -format cpp|go -stop_after <int>\n");
        printf("Usage:\n\n[ECO]\n./eco -train net.txt -field field.txt -save rep.txt -dimensions 64 -sample_times 10 "
               "-negative_samples 5 -alpha 0.025 -reg 0.01 -threads 1\n");
        return 0;
    }
    char network_file[4096] = "", rep_file[4096] = "", field_file[4096] = "";
    int dimensions = 64, negative_samples = 5, sample_times = 10, threads = 1, device = 0, gpus = 1, fmt = 0;
    int mode = SMORE_HYBRID;
    unsigned long long seed = 1, stop_after = 0;
    double init_alpha = 0.025, reg = 0.01;
    if ((i = ArgPos("-train", argc, argv)) > 0) snprintf(network_file, sizeof network_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-save", argc, argv)) > 0) snprintf(rep_file, sizeof rep_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-field", argc, argv)) > 0) snprintf(field_file, sizeof field_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-dimensions", argc, argv)) > 0) dimensions = atoi(argv[i + 1]);
    if ((i = ArgPos("-negative_samples", argc, argv)) > 0) negative_samples = atoi(argv[i + 1]);
    if ((i = ArgPos("-sample_times", argc, argv)) > 0) sample_times = atoi(argv[i + 1]);
    if ((i = ArgPos("-alpha", argc, argv)) > 0) init_alpha = atof(argv[i + 1]);
    if ((i = ArgPos("-reg", argc, argv)) > 0) reg = atof(argv[i + 1]);
    if ((i = ArgPos("-threads", argc, argv)) > 0) threads = atoi(argv[i + 1]);
    if ((i = ArgPos("-device", argc, argv)) > 0) device = atoi(argv[i + 1]);
    if ((i = ArgPos("-gpus", argc, argv)) > 0) gpus = atoi(argv[i + 1]);
    if ((i = ArgPos("-mode", argc, argv)) > 0) mode = mode_of(argv[i + 1]);
    if ((i = ArgPos("-seed", argc, argv)) > 0) seed = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-stop_after", argc, argv)) > 0) stop_after = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-format", argc, argv)) > 0) fmt = !strcmp(argv[i + 1], "go");
    if (gpus > 1) {
        fprintf(stderr, "eco: -gpus %d: ECO runs on one GPU (no multi-GPU schedule for it)\n", gpus);
        return 1;
    }

    Run run = open_run(device, 1);
    smore_ctx* ctx = run.ctx;
    // ECO() sets negative_method "no_degrees" (src/model/ECO.cpp:4-7); LoadEdgeList(file, 1)
    run_load(run, network_file, 1, SMORE_VM_OUT_DEGREES, SMORE_NM_NO_DEGREES);
    print_graph(ctx);
    SMORE_CLI_CHECK(ctx, smore_load_field_meta(ctx, field_file));
    int nfields = 0;
    int64_t meta_lines = 0, meta_unknown = 0;
    SMORE_CLI_CHECK(ctx, smore_get_fields(ctx, nullptr, &nfields));
    SMORE_CLI_CHECK(ctx, smore_field_meta_info(ctx, &meta_lines, &meta_unknown));
    printf("Meta Data Preview:\n\t# of meta data:\t\t%lld\nMeta Data Loading:\n", (long long)meta_lines);
    if (meta_unknown) printf("\t%lld vertices are not in given network\n", (long long)meta_unknown);
    printf("\t# of field:\t\t%d\n", nfields);
    printf("Model Setting:\n\tdimension:\t\t%d\n", dimensions);
    run_alloc(run, dimensions, 1);
    // Init: w_vertex takes the even draws of the rand() stream, w_ignore (never used) the odd ones
    SMORE_CLI_CHECK(ctx, smore_init_table_glibc_unscaled(ctx, SMORE_W, 0, 2));
    run_replicate(run);
    printf("Model:\n\t[ECO]\nLearning Parameters:\n\tsample_times:\t\t%d\n\tnegative_samples:\t%d\n\talpha:\t\t\t%g\n"
           "\tregularization:\t\t%g\n\tworkers:\t\t%d\nStart Training:\n", sample_times, negative_samples, init_alpha, reg,
           threads);
    const unsigned long long total = (unsigned long long)sample_times * 1000000ull, chunk = 1ull << 26;
    const unsigned long long end = stop_after && stop_after < total ? stop_after : total;
    for (unsigned long long done = 0; done < end;) {
        const unsigned long long n = end - done < chunk ? end - done : chunk;
        SMORE_CLI_CHECK(ctx, smore_train_eco(ctx, done, n, total, negative_samples, init_alpha, reg, seed, mode));
        done += n;
        printf("\tProgress: %.3f %%%c", (double)done / total * 100, 13);
        fflush(stdout);
    }
    printf("\tProgress: %.2f %%\n", (double)end / total * 100);
    save(ctx, rep_file, fmt);
    run_close(run);
    return 0;
}

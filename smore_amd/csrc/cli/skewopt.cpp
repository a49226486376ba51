// skewopt -- flag-compatible replacement of cli/skewopt.cpp (SPR, the
// reference's Skew-OPT: per sample one positive pair and sixteen negatives
// through UpdateSBPRPair; src/model/SkewOPT.cpp:55-110, src/proNet.cpp:1517-1566).
// Extra flags: -device, -mode atomic|hybrid|serial, -seed, -format cpp|go,
// -samples <n> (the exact number of samples instead of sample_times x 10^6).
// One GPU only.
#include "cli_common.h"

int main(int argc, char** argv) {
    int i;
    if (argc == 1) {
        printf("[smore-mi355x] Skew-OPT\n\nOptions Description:\n");
        printf("\t-train <string>\n\t-save <string>\n\t-dimensions <int> (64)\n\t-sample_times <int> (10, x10^6)\n");
        printf("\t-threads <int>\n\t-reg <float> (0.01, unused by the rule)\n\t-xi <float> (10.0)\n\t-omega <float> (3.0)\n");
        printf("\t-eta <int> (3)\n\t-alpha <float> (0.025)\n");
        printf("\t-device <int> -mode atomic|hybrid|serial -seed <int> -format cpp|go -samples <int>\n");
        printf("Usage:\n\n[SkewOPT]\n./skewopt -train net.txt -save rep.txt -dimensions 64 -sample_times 10 -alpha 0.025 "
               "-threads 1\n");
        return 0;
    }
    char network_file[4096] = "", rep_file[4096] = "";
    int dimensions = 64, sample_times = 10, threads = 1, eta = 3, device = 0, gpus = 1, fmt = 0;
    int mode = SMORE_HYBRID;
    unsigned long long seed = 1, samples = 0;
    double init_alpha = 0.025, reg = 0.01, xi = 10.0, omega = 3.0;
    if ((i = ArgPos("-train", argc, argv)) > 0) snprintf(network_file, sizeof network_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-save", argc, argv)) > 0) snprintf(rep_file, sizeof rep_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-dimensions", argc, argv)) > 0) dimensions = atoi(argv[i + 1]);
    if ((i = ArgPos("-sample_times", argc, argv)) > 0) sample_times = atoi(argv[i + 1]);
    if ((i = ArgPos("-reg", argc, argv)) > 0) reg = atof(argv[i + 1]);
    if ((i = ArgPos("-xi", argc, argv)) > 0) xi = atof(argv[i + 1]);
    if ((i = ArgPos("-omega", argc, argv)) > 0) omega = atof(argv[i + 1]);
    if ((i = ArgPos("-eta", argc, argv)) > 0) eta = atoi(argv[i + 1]);
    if ((i = ArgPos("-alpha", argc, argv)) > 0) init_alpha = atof(argv[i + 1]);
    if ((i = ArgPos("-threads", argc, argv)) > 0) threads = atoi(argv[i + 1]);
    if ((i = ArgPos("-device", argc, argv)) > 0) device = atoi(argv[i + 1]);
    if ((i = ArgPos("-gpus", argc, argv)) > 0) gpus = atoi(argv[i + 1]);
    if ((i = ArgPos("-mode", argc, argv)) > 0) mode = mode_of(argv[i + 1]);
    if ((i = ArgPos("-seed", argc, argv)) > 0) seed = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-samples", argc, argv)) > 0) samples = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-format", argc, argv)) > 0) fmt = !strcmp(argv[i + 1], "go");
    if (gpus > 1) {
        fprintf(stderr, "skewopt: -gpus %d: Skew-OPT runs on one GPU (no multi-GPU schedule for it)\n", gpus);
        return 1;
    }

    Run run = open_run(device, 1);
    smore_ctx* ctx = run.ctx;
    // SPR() sets negative_method "no_degrees" (src/model/SkewOPT.cpp:4-7); LoadEdgeList(file, 0)
    run_load(run, network_file, 0, SMORE_VM_OUT_DEGREES, SMORE_NM_NO_DEGREES);
    print_graph(ctx);
    printf("Model Setting:\n\tdimension:\t\t%d\n", dimensions);
    run_alloc(run, dimensions, 1);
    SMORE_CLI_CHECK(ctx, smore_init_table_glibc_offset(ctx, SMORE_W, 0, 0.01));
    run_replicate(run);
    printf("Model:\n\t[Skew-OPT]\nLearning Parameters:\n\tsample_times:\t\t%d\n\talpha:\t\t\t%g\n"
           "\tregularization:\t\t%g\n\txi:\t\t\t%g\n\tomega:\t\t\t%g\n\teta:\t\t\t%d\n\tworkers:\t\t%d\nStart Training:\n",
           sample_times, init_alpha, reg, xi, omega, eta, threads);
    const unsigned long long total = samples ? samples : (unsigned long long)sample_times * 1000000ull, chunk = 1ull << 26;
    for (unsigned long long done = 0; done < total;) {
        const unsigned long long n = total - done < chunk ? total - done : chunk;
        SMORE_CLI_CHECK(ctx, smore_train_skewopt(ctx, done, n, total, init_alpha, xi, omega, eta, seed, mode));
        done += n;
        printf("\tProgress: %.3f %%%c", (double)done / total * 100, 13);
        fflush(stdout);
    }
    printf("\tProgress: 100.00 %%\n");
    save(ctx, rep_file, fmt);
    run_close(run);
    return 0;
}

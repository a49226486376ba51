// textgcndev -- flag-compatible replacement of cli/textgcndev.cpp (the bag-of-words
// event rule: per sample a field-0 user, num_events events and num_words words of
// each, the words' w_context rows summed into a bag, W[event] and ten uniform
// field-1 rows per iteration stepped against the bag and against W[user];
// src/model/TEXTGCNdev.cpp:71-126).  The defaults are the reference's as coded
// (sample_times 10; its help text says 5).  Extra flags: -device, -mode
// atomic|hybrid|serial, -seed, -format cpp|go, -stop_after <n> (run only the first
// n samples of the sample_times x 10^6 schedule).  One GPU only.
#include "cli_common.h"

int main(int argc, char** argv) {
    int i;
    if (argc == 1) {
        printf("[smore-mi355x] TEXTGCNdev (textgcndev)\n\nOptions Description:\n");
        printf("\t-train <string>\n\t-save <string>\n\t-field <string>\n\t-dimensions <int> (64)\n\t-undirected <int> (1)\n");
        printf("\t-num_events <int> (1)\n\t-num_words <int> (5)\n\t-sample_times <int> (10, x10^6)\n");
        printf("\t-reg <float> (0.01)\n\t-alpha <float> (0.025)\n\t-threads <int>\n");
        printf("\t-device <int> -mode atomic|hybrid|serial -seed <int> -format cpp|go -stop_after <int>\n");
        printf("Usage:\n./textgcndev -train net.txt -field field.txt -save rep.txt -undirected 1 -dimensions 64 -reg 0.01 "
               "-sample_times 10 -num_events 1 -num_words 5 -alpha 0.025 -threads 1\n");
        return 0;
    }
    char network_file[4096] = "", rep_file[4096] = "", field_file[4096] = "";
    int dimensions = 64, undirected = 1, num_events = 1, num_words = 5, sample_times = 10, threads = 1;
    int device = 0, gpus = 1, fmt = 0, mode = SMORE_HYBRID;
    unsigned long long seed = 1, stop_after = 0;
    double init_alpha = 0.025, reg = 0.01;
    if ((i = ArgPos("-train", argc, argv)) > 0) snprintf(network_file, sizeof network_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-save", argc, argv)) > 0) snprintf(rep_file, sizeof rep_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-field", argc, argv)) > 0) snprintf(field_file, sizeof field_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-undirected", argc, argv)) > 0) undirected = atoi(argv[i + 1]);
    if ((i = ArgPos("-dimensions", argc, argv)) > 0) dimensions = atoi(argv[i + 1]);
    if ((i = ArgPos("-num_events", argc, argv)) > 0) num_events = atoi(argv[i + 1]);
    if ((i = ArgPos("-num_words", argc, argv)) > 0) num_words = atoi(argv[i + 1]);
    if ((i = ArgPos("-sample_times", argc, argv)) > 0) sample_times = atoi(argv[i + 1]);
    if ((i = ArgPos("-reg", argc, argv)) > 0) reg = atof(argv[i + 1]);
    if ((i = ArgPos("-alpha", argc, argv)) > 0) init_alpha = atof(argv[i + 1]);
    if ((i = ArgPos("-threads", argc, argv)) > 0) threads = atoi(argv[i + 1]);
    if ((i = ArgPos("-device", argc, argv)) > 0) device = atoi(argv[i + 1]);
    if ((i = ArgPos("-gpus", argc, argv)) > 0) gpus = atoi(argv[i + 1]);
    if ((i = ArgPos("-mode", argc, argv)) > 0) mode = mode_of(argv[i + 1]);
    if ((i = ArgPos("-seed", argc, argv)) > 0) seed = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-stop_after", argc, argv)) > 0) stop_after = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-format", argc, argv)) > 0) fmt = !strcmp(argv[i + 1], "go");
    if (gpus > 1) {
        fprintf(stderr, "textgcndev: -gpus %d: TEXTGCNdev runs on one GPU (no multi-GPU schedule for it)\n", gpus);
        return 1;
    }

    Run run = open_run(device, 1);
    smore_ctx* ctx = run.ctx;
    // TEXTGCNdev(): proNet's defaults (out_degrees sources; the negative table is never used)
    run_load(run, network_file, undirected, SMORE_VM_OUT_DEGREES, SMORE_NM_DEGREES);
    print_graph(ctx);
    SMORE_CLI_CHECK(ctx, smore_load_field_meta(ctx, field_file));
    int nfields = 0;
    int64_t meta_lines = 0, meta_unknown = 0, V = 0;
    SMORE_CLI_CHECK(ctx, smore_get_fields(ctx, nullptr, &nfields));
    SMORE_CLI_CHECK(ctx, smore_field_meta_info(ctx, &meta_lines, &meta_unknown));
    SMORE_CLI_CHECK(ctx, smore_graph_info(ctx, &V, nullptr));
    printf("Meta Data Preview:\n\t# of meta data:\t\t%lld\nMeta Data Loading:\n", (long long)meta_lines);
    if (meta_unknown) printf("\t%lld vertices are not in given network\n", (long long)meta_unknown);
    printf("\t# of field:\t\t%d\n", nfields);
    printf("Model Setting:\n\tdimension:\t\t%d\n", dimensions);
    run_alloc(run, dimensions, 2);
    // Init: w_vertex whole, then w_context, from one rand() stream
    SMORE_CLI_CHECK(ctx, smore_init_table_glibc(ctx, 0, 0));
    SMORE_CLI_CHECK(ctx, smore_init_table_glibc(ctx, 1, (uint64_t)V * (uint64_t)dimensions));
    run_replicate(run);
    printf("Model:\n\t[TEXTGCNdev]\nLearning Parameters:\n\tsample_times:\t\t%d\n\tnegative_samples:\tfixed\n\tnum_events:\t%d\n"
           "\tnum_words:\t%d\n\tregularization:\t\t%g\n\talpha:\t\t\t%g\n\tworkers:\t\t%d\nStart Training:\n",
           sample_times, num_events, num_words, reg, init_alpha, threads);
    const unsigned long long total = (unsigned long long)sample_times * 1000000ull, chunk = 1ull << 26;
    const unsigned long long end = stop_after && stop_after < total ? stop_after : total;
    for (unsigned long long done = 0; done < end;) {
        const unsigned long long n = end - done < chunk ? end - done : chunk;
        SMORE_CLI_CHECK(ctx, smore_train_cbowdev(ctx, done, n, total, num_events, num_words, init_alpha, reg, seed, mode));
        done += n;
        printf("\tProgress: %.3f %%%c", (double)done / total * 100, 13);
        fflush(stdout);
    }
    printf("\tProgress: %.2f %%\n", (double)end / total * 100);
    (void)save;   // the model's own saver below instead of the one-table one
    printf("Save Model:\n");
    SMORE_CLI_CHECK(ctx, smore_save_weights_textgcndev(ctx, rep_file, fmt));
    printf("\tSave to <%s>\n", rep_file);
    run_close(run);
    return 0;
}

// cse_cli.h -- the shared body of bin/nemf and bin/nerank: flag-compatible
// replacements of cli/nemf.cpp and cli/nerank.cpp (CSE: per sample a field-0
// source, two neighbourhood passes and a direct user-item term on four tables;
// src/model/NEMF.cpp:87-149, src/model/NERANK.cpp:87-148).  Extra flags:
// -device, -mode atomic|hybrid|serial, -seed, -format cpp|go, -stop_after <n>
// (run only the first n samples of the sample_times x 10^6 schedule).  One GPU only.
#pragma once
#include "cli_common.h"

static int cse_main(int argc, char** argv, int rank) {
    const char* prog = rank ? "nerank" : "nemf";
    const char* tag = rank ? "NERANK" : "NEMF";
    int i;
    if (argc == 1) {
        printf("[smore-mi355x] CSE (%s)\n\nOptions Description:\n", prog);
        printf("\t-train <string>\n\t-save <string>\n\t-field <string>\n\t-dimensions <int> (64)\n");
        printf("\t-sample_times <int> (10, x10^6)\n\t-walk_steps <int> (5)\n\t-alpha <float> (0.025)\n\t-threads <int>\n");
        printf("\t-device <int> -mode atomic|hybrid|serial -seed <int> -format cpp|go -stop_after <int>\n");
        printf("Usage:\n\n[%s]\n./%s -train net.txt -field field.txt -save rep.txt -dimensions 64 -sample_times 10 "
               "-walk_steps 5 -alpha 0.025 -threads 1\n", tag, prog);
        return 0;
    }
    char network_file[4096] = "", rep_file[4096] = "", field_file[4096] = "";
    int dimensions = 64, sample_times = 10, walk_steps = 5, threads = 1, device = 0, gpus = 1, fmt = 0;
    int mode = SMORE_HYBRID;
    unsigned long long seed = 1, stop_after = 0;
    double init_alpha = 0.025;
    if ((i = ArgPos("-train", argc, argv)) > 0) snprintf(network_file, sizeof network_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-save", argc, argv)) > 0) snprintf(rep_file, sizeof rep_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-field", argc, argv)) > 0) snprintf(field_file, sizeof field_file, "%s", argv[i + 1]);
    if ((i = ArgPos("-dimensions", argc, argv)) > 0) dimensions = atoi(argv[i + 1]);
    if ((i = ArgPos("-sample_times", argc, argv)) > 0) sample_times = atoi(argv[i + 1]);
    if ((i = ArgPos("-walk_steps", argc, argv)) > 0) walk_steps = atoi(argv[i + 1]);
    if ((i = ArgPos("-alpha", argc, argv)) > 0) init_alpha = atof(argv[i + 1]);
    if ((i = ArgPos("-threads", argc, argv)) > 0) threads = atoi(argv[i + 1]);
    if ((i = ArgPos("-device", argc, argv)) > 0) device = atoi(argv[i + 1]);
    if ((i = ArgPos("-gpus", argc, argv)) > 0) gpus = atoi(argv[i + 1]);
    if ((i = ArgPos("-mode", argc, argv)) > 0) mode = mode_of(argv[i + 1]);
    if ((i = ArgPos("-seed", argc, argv)) > 0) seed = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-stop_after", argc, argv)) > 0) stop_after = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-format", argc, argv)) > 0) fmt = !strcmp(argv[i + 1], "go");
    if (gpus > 1) {
        fprintf(stderr, "%s: -gpus %d: CSE runs on one GPU (no multi-GPU schedule for it)\n", prog, gpus);
        return 1;
    }

    Run run = open_run(device, 1);
    smore_ctx* ctx = run.ctx;
    // NEMF() / NERANK(): out_degrees sources, degrees negatives; LoadEdgeList(file, 1)
    run_load(run, network_file, 1, SMORE_VM_OUT_DEGREES, SMORE_NM_DEGREES);
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
    run_alloc(run, dimensions, 4);   // WU, WI, CU, CI (zero)
    SMORE_CLI_CHECK(ctx, smore_init_tables_glibc_pair(ctx, 0, 1, 0));
    run_replicate(run);
    printf("Model:\n\t[%s]\nLearning Parameters:\n\tsample_times:\t\t%d\n\talpha:\t\t\t%g\n"
           "\twalk steps:\t\t%d\n\tworkers:\t\t%d\nStart Training[1]:\n", tag, sample_times, init_alpha, walk_steps, threads);
    const unsigned long long total = (unsigned long long)sample_times * 1000000ull, chunk = 1ull << 26;
    const unsigned long long end = stop_after && stop_after < total ? stop_after : total;
    for (unsigned long long done = 0; done < end;) {
        const unsigned long long n = end - done < chunk ? end - done : chunk;
        SMORE_CLI_CHECK(ctx, smore_train_cse(ctx, rank, done, n, total, walk_steps, init_alpha, seed, mode));
        done += n;
        printf("\tProgress: %.3f %%%c", (double)done / total * 100, 13);
        fflush(stdout);
    }
    printf("\tProgress: %.2f %%\n", (double)end / total * 100);
    (void)save;   // the per-field saver below instead of the one-table one
    // SaveWeights: WU rows for field 0, WI rows for field 1, the name alone for any other field
    std::vector<int> tof((size_t)(nfields > 2 ? nfields : 2), -1);
    tof[0] = 0;
    tof[1] = 1;
    printf("Save Model:\n");
    SMORE_CLI_CHECK(ctx, smore_save_weights_fields(ctx, tof.data(), (int)tof.size(), rep_file, fmt));
    printf("\tSave to <%s>\n", rep_file);
    run_close(run);
    return 0;
}

// hoprec -- flag-compatible replacement of cli/hoprec.cpp (HBPR, the
// reference's HOP-REC: per sample a field-0 source and walk_steps
// UpdateFBPRPair steps; src/model/HBPR.cpp:63-131, src/proNet.cpp:1458-1515).
// Extra flags: -device, -mode atomic|hybrid|serial, -seed, -format cpp|go,
// -samples <n> (the exact number of samples instead of sample_times x 10^6).
// One GPU only.
#include "cli_common.h"

int main(int argc, char** argv) {
    int i;
    if (argc == 1) {
        printf("[smore-mi355x] HOP-REC\n\nOptions Description:\n");
        printf("\t-train <string>\n\t-save <string>\n\t-field <string>\n\t-dimensions <int> (64)\n");
        printf("\t-sample_times <int> (10, x10^6)\n\t-walk_steps <int> (5)\n\t-alpha <float> (0.025)\n\t-threads <int>\n");
        printf("\t-device <int> -mode atomic|hybrid|serial -seed <int> -format cpp|go -samples <int>\n");
        printf("Usage:\n\n[HBPR]\n./hoprec -train net.txt -field field.txt -save rep.txt -dimensions 64 -sample_times 10 "
               "-alpha 0.025 -threads 1\n");
        return 0;
    }
    char network_file[4096] = "", rep_file[4096] = "", field_file[4096] = "";
    int dimensions = 64, sample_times = 10, walk_steps = 5, threads = 1, device = 0, gpus = 1, fmt = 0;
    int mode = SMORE_HYBRID;
    unsigned long long seed = 1, samples = 0;
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
    if ((i = ArgPos("-samples", argc, argv)) > 0) samples = strtoull(argv[i + 1], 0, 10);
    if ((i = ArgPos("-format", argc, argv)) > 0) fmt = !strcmp(argv[i + 1], "go");
    if (gpus > 1) {
        fprintf(stderr, "hoprec: -gpus %d: HOP-REC runs on one GPU (no multi-GPU schedule for it)\n", gpus);
        return 1;
    }

    Run run = open_run(device, 1);
    smore_ctx* ctx = run.ctx;
    // HBPR() sets negative_method "no_degrees" (src/model/HBPR.cpp:4-7); LoadEdgeList(file, 1)
    run_load(run, network_file, 1, SMORE_VM_OUT_DEGREES, SMORE_NM_NO_DEGREES);
    print_graph(ctx);
    SMORE_CLI_CHECK(ctx, smore_load_field_meta(ctx, field_file));
    int nfields = 0;
    int64_t meta_lines = 0, meta_unknown = 0;
    SMORE_CLI_CHECK(ctx, smore_get_fields(ctx, nullptr, &nfields));
    SMORE_CLI_CHECK(ctx, smore_field_meta_info(ctx, &meta_lines, &meta_unknown));
    printf("Meta Data Preview:\n\t# of meta data:\t\t%lld\nMeta Data Loading:\n", (long long)meta_lines);
    // the reference prints "vertex <name> is not in given network" per such line
    if (meta_unknown) printf("\t%lld vertices are not in given network\n", (long long)meta_unknown);
    printf("\t# of field:\t\t%d\n", nfields);
    printf("Model Setting:\n\tdimension:\t\t%d\n", dimensions);
    run_alloc(run, dimensions, 1);
    SMORE_CLI_CHECK(ctx, smore_init_table_glibc(ctx, SMORE_W, 0));
    run_replicate(run);
    printf("Model:\n\t[HBPR]\nLearning Parameters:\n\tsample_times:\t\t%d\n\talpha:\t\t\t%g\n"
           "\twalk steps:\t\t%d\n\tworkers:\t\t%d\nStart Training:\n", sample_times, init_alpha, walk_steps, threads);
    const unsigned long long total = samples ? samples : (unsigned long long)sample_times * 1000000ull, chunk = 1ull << 26;
    for (unsigned long long done = 0; done < total;) {
        const unsigned long long n = total - done < chunk ? total - done : chunk;
        SMORE_CLI_CHECK(ctx, smore_train_hoprec(ctx, done, n, total, walk_steps, init_alpha, seed, mode));
        done += n;
        printf("\tProgress: %.3f %%%c", (double)done / total * 100, 13);
        fflush(stdout);
    }
    printf("\tProgress: 100.00 %%\n");
    save(ctx, rep_file, fmt);
    run_close(run);
    return 0;
}

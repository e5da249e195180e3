/* offline_batch_profile_switch.c — a headphone profile changed at a cue point, inside the batch entries: half of the streams fade from
 * preset A to preset B over 20 ms at a given second, the others go on untouched.
 *
 *   N streams of interleaved 7.1 float32 in host memory  ->  HeSuVi HRIR preset  ->  equalizer preset A on every stream
 *   ->  at second `cue`: the odd streams fade to preset B (aw_spatializer_set_equalizer_target), the even ones are AW_EQ_KEEP
 *   ->  N stereo float32 streams.
 *
 * The programme is rendered in calls of one second, as a host does that decodes while it renders.  An install
 * (aw_spatializer_set_equalizer) at the cue would click and start B's filters cold; leaving the batch entries for aw_eq would take the
 * equalizer out from in front of the meters, the gain and the limiter.  The target is published between two calls and begins with the
 * first frame of the next one: the stage runs both presets on the fading streams for 960 frames and mixes them, every later stage sees
 * the result, and the streams that keep their profile are not touched: their filter state goes on as if nothing had happened.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_profile_switch.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_profile_switch
 *   ./offline_batch_profile_switch tests/golden/hrtf/RoomSH1.0.wav "tests/golden/eq/Bass Booster.txt" "tests/golden/eq/Treble Reducer.txt" [streams] [seconds] [cue] [out.f32]
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "airwave_hip.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        aw_status st_ = (call);                                                                       \
        if (st_ != AW_OK) {                                                                           \
            fprintf(stderr, "%s: %s (%s)\n", #call, aw_status_string(st_), aw_last_error_message()); \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

/* an Equalizer APO preset file -> a definition */
static int load_preset(const char *path, aw_eq_definition **out) {
    static char text[65536], issues[1024];
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return 1; }
    const size_t n = fread(text, 1, sizeof text, f);
    fclose(f);
    if (aw_eq_parse(text, n, out, issues, sizeof issues) != AW_OK) { fprintf(stderr, "%s: %s\n", path, issues); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s hrir.wav preset_a.txt preset_b.txt [streams] [seconds] [cue second] [out.f32]\n", argv[0]);
        return 2;
    }
    const int streams = argc > 4 ? atoi(argv[4]) : 16;
    const int seconds = argc > 5 ? atoi(argv[5]) : 4;
    const int cue = argc > 6 ? atoi(argv[6]) : seconds / 2;
    const int64_t rate = 48000, call = rate;                          /* calls of one second */
    const int channels = 8;
    if (streams < 1 || seconds < 1 || cue < 0 || cue > seconds) return 2;

    aw_context *ctx = NULL;
    aw_layout *layout = NULL;
    aw_spatializer *sp = NULL;
    CHECK(aw_context_create(0, &ctx));
    CHECK(aw_layout_detect(channels, &layout));
    CHECK(aw_preset_activate(ctx, argv[1], (double)rate, layout, NULL, streams, &sp, NULL));
    aw_eq_definition *a = NULL, *b = NULL;
    int32_t *which = (int32_t *)calloc((size_t)streams, sizeof *which);
    if (!which || load_preset(argv[2], &a) || load_preset(argv[3], &b)) return 1;
    CHECK(aw_spatializer_set_equalizer(sp, (const aw_eq_definition *const *)&a, 1, NULL));      /* preset A on every stream */
    CHECK(aw_spatializer_reserve_host(sp, call));

    /* one second of every stream at a time, [stream][frame][channel]; the output file is [stream][second][frame][2] put in order below */
    const size_t n_in = (size_t)streams * (size_t)call * channels, n_out = (size_t)streams * (size_t)call * 2;
    float *in = NULL, *out = NULL;
    CHECK(aw_host_alloc_pinned(ctx, n_in * sizeof(float), (void **)&in));
    CHECK(aw_host_alloc_pinned(ctx, n_out * sizeof(float), (void **)&out));
    float *programme = (float *)malloc((size_t)seconds * n_out * sizeof(float));
    if (!programme) return 1;
    uint32_t s = 12345u;
    for (int sec = 0; sec < seconds; ++sec) {
        if (sec == cue) {                                             /* the cue: odd streams to preset B, the even ones keep theirs */
            for (int i = 0; i < streams; ++i) which[i] = (i & 1) ? 0 : AW_EQ_KEEP;
            CHECK(aw_spatializer_set_equalizer_target(sp, (const aw_eq_definition *const *)&b, 1, which));
            printf("second %d: target published (pending %lld)\n", sec, (long long)aw_spatializer_info(sp, 28));
        }
        for (size_t k = 0; k < n_in; ++k) {                           /* white noise, the same level on every stream */
            s = s * 1664525u + 1013904223u;
            in[k] = ((float)(s >> 8) / 16777216.0f - 0.5f) * 0.1f;
        }
        CHECK(aw_spatializer_process_host(sp, in, out, call));
        printf("second %d: presets held %lld, fade frames left %lld, pending %lld\n", sec, (long long)aw_spatializer_info(sp, 25),
               (long long)aw_spatializer_info(sp, 27), (long long)aw_spatializer_info(sp, 28));
        for (int i = 0; i < streams; ++i)
            memcpy(programme + ((size_t)i * (size_t)seconds + (size_t)sec) * (size_t)call * 2, out + (size_t)i * (size_t)call * 2, (size_t)call * 2 * sizeof(float));
    }
    printf("streams %d seconds %d cue %d: odd streams switched, even streams kept\n", streams, seconds, cue);
    if (argc > 7) {                                                   /* [stream][seconds * 48000][2] */
        FILE *f = fopen(argv[7], "wb");
        const size_t n = (size_t)streams * (size_t)seconds * (size_t)call * 2;
        if (!f || fwrite(programme, sizeof(float), n, f) != n) { fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
        fclose(f);
    }

    aw_eq_definition_destroy(a);
    aw_eq_definition_destroy(b);
    free(which);
    free(programme);
    CHECK(aw_host_free_pinned(ctx, in));
    CHECK(aw_host_free_pinned(ctx, out));
    aw_spatializer_destroy(sp);
    aw_layout_destroy(layout);
    aw_context_destroy(ctx);
    return 0;
}

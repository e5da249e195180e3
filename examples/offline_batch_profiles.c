/* offline_batch_profiles.c — one headphone preset per stream in front of the whole output chain: equalize, measure the loudness, then one
 * gain per stream behind a look-ahead true-peak limiter, then 16-bit output.
 *
 *   N streams of interleaved 7.1 float32 in host memory  ->  HeSuVi HRIR preset  ->  one of two equalizer presets, alternating by stream
 *   ->  N stereo s16 streams at -16 LUFS, at most -1 dBTP.
 *
 * The reference ties an equalizer preset to each output device (its device profiles) and runs it behind the spatializer.  A batch whose
 * streams go to different headphones cannot fold the equalizer into the shared HRIR, and an equalizer run as a second call would come
 * after the meters and the limiter: the loudness would be measured on the wrong signal and the ceiling would not hold.
 * aw_spatializer_set_equalizer puts the cascade between the convolution and the first meter instead, so this is offline_batch_limiter.c
 * with three more calls: parse two presets, install them with a stream -> preset map, destroy the definitions.  Both passes equalize;
 * aw_spatializer_reset between them starts the filters again from zero.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_profiles.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_profiles
 *   ./offline_batch_profiles tests/golden/hrtf/RoomSH1.0.wav "tests/golden/eq/Bass Booster.txt" "tests/golden/eq/Treble Reducer.txt" [streams] [seconds] [out.s16]
 */
#include <math.h>
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
        fprintf(stderr, "usage: %s hrir.wav preset_a.txt preset_b.txt [streams] [seconds] [out.s16]\n", argv[0]);
        return 2;
    }
    const int streams = argc > 4 ? atoi(argv[4]) : 16;
    const double seconds = argc > 5 ? atof(argv[5]) : 2.0;
    const int64_t frames = (int64_t)(seconds * 48000.0);
    const int channels = 8;
    const double target_lufs = -16.0, ceiling_dbtp = -1.0;
    const int32_t attack = 64, hold = 128;
    if (streams < 1 || frames < 1) return 2;

    aw_context *ctx = NULL;
    aw_layout *layout = NULL;
    aw_spatializer *sp = NULL;
    CHECK(aw_context_create(0, &ctx));
    CHECK(aw_layout_detect(channels, &layout));
    CHECK(aw_preset_activate(ctx, argv[1], 48000.0, layout, NULL, streams, &sp, NULL));
    /* the two presets, alternating by stream; the spatializer keeps tables of its own, so the definitions can go at once */
    aw_eq_definition *presets[2] = {NULL, NULL};
    int32_t *which = (int32_t *)calloc((size_t)streams, sizeof *which);
    if (!which || load_preset(argv[2], &presets[0]) || load_preset(argv[3], &presets[1])) return 1;
    for (int i = 0; i < streams; ++i) which[i] = i & 1;
    CHECK(aw_spatializer_set_equalizer(sp, (const aw_eq_definition *const *)presets, 2, which));
    const int filters[2] = {aw_eq_definition_filter_count(presets[0]), aw_eq_definition_filter_count(presets[1])};
    aw_eq_definition_destroy(presets[0]);
    aw_eq_definition_destroy(presets[1]);
    CHECK(aw_spatializer_set_loudness(sp, 1, seconds));               /* the records are allocated now, not in process */
    CHECK(aw_spatializer_set_metering(sp, 1));                        /* the per-stream clip counts of pass two */
    CHECK(aw_spatializer_set_limiter(sp, 1, (float)pow(10.0, ceiling_dbtp / 20.0), attack, hold));
    const int64_t delay = aw_spatializer_info(sp, 24), padded = frames + delay;
    CHECK(aw_spatializer_set_limiter(sp, 0, 0.0f, 0, 0));             /* (pass one measures; the limiter's buffers stay) */
    CHECK(aw_spatializer_reserve_pcm(sp, padded, AW_SAMPLE_F32, AW_SAMPLE_S16));

    /* the file, and behind every stream the D frames of zeros that flush the limiter */
    const size_t n_in = (size_t)streams * (size_t)padded * channels, n_out = (size_t)streams * (size_t)padded * 2;
    float *in = NULL, *scratch = NULL;
    int16_t *out = NULL;
    CHECK(aw_host_alloc_pinned(ctx, n_in * sizeof(float), (void **)&in));
    CHECK(aw_host_alloc_pinned(ctx, n_out * sizeof(float), (void **)&scratch));
    CHECK(aw_host_alloc_pinned(ctx, n_out * sizeof(int16_t), (void **)&out));
    memset(in, 0, n_in * sizeof(float));
    uint32_t s = 12345u;                                              /* quiet to loud from stream to stream */
    for (int i = 0; i < streams; ++i) {
        const float level = 0.01f + 0.5f * (float)i / (float)streams;
        float *x = in + (size_t)i * (size_t)padded * channels;
        for (size_t k = 0; k < (size_t)frames * channels; ++k) {
            s = s * 1664525u + 1013904223u;
            x[k] = ((float)(s >> 8) / 16777216.0f - 0.5f) * level;
        }
        /* one click per stream, sixteen times the noise's largest sample on every channel: under a tenth of a dB in LUFS over two
         * seconds, several dB over the ceiling once the stream is at its target — what the limiter is for */
        if (frames > 20000)
            for (int c = 0; c < channels; ++c) x[(size_t)20000 * channels + c] = 8.0f * level;
    }

    /* pass one: measure the EQUALIZED streams (the zeros behind the file add silence, which the gates drop) */
    CHECK(aw_spatializer_process_host(sp, in, scratch, padded));
    aw_stream_loudness *ld = (aw_stream_loudness *)calloc((size_t)streams, sizeof *ld);
    aw_stream_limiter *lim = (aw_stream_limiter *)calloc((size_t)streams, sizeof *lim);
    aw_stream_levels *lv = (aw_stream_levels *)calloc((size_t)streams, sizeof *lv);
    float *gains = (float *)calloc((size_t)streams, sizeof *gains);
    if (!ld || !lim || !lv || !gains) return 1;
    CHECK(aw_spatializer_get_loudness(sp, 0, streams, ld));
    for (int i = 0; i < streams; ++i)
        if (aw_loudness_gain(ld[i].integrated_lufs, target_lufs, &gains[i]) != AW_OK) gains[i] = 1.0f;     /* silence: nothing to bring anywhere */

    /* pass two: the same input from the start (the reset zeroes the equalizer's state too), fixed gains, the limiter, dithered s16 */
    CHECK(aw_spatializer_reset(sp));
    CHECK(aw_spatializer_set_loudness(sp, 0, 0.0));
    CHECK(aw_spatializer_set_gain(sp, AW_GAIN_FIXED, gains, streams, 0.0f));
    CHECK(aw_spatializer_set_limiter(sp, 1, (float)pow(10.0, ceiling_dbtp / 20.0), attack, hold));
    CHECK(aw_spatializer_set_dither(sp, AW_DITHER_TPDF, 1, 0));
    uint64_t clipped = 0;
    CHECK(aw_spatializer_process_host_pcm(sp, in, AW_SAMPLE_F32, out, AW_SAMPLE_S16, padded, &clipped));
    CHECK(aw_spatializer_get_levels(sp, 0, streams, lv));
    CHECK(aw_spatializer_get_limiter(sp, 0, streams, lim));
    printf("presets %lld (%d and %d filters, at most %lld enabled)\n", (long long)aw_spatializer_info(sp, 25), filters[0], filters[1],
           (long long)aw_spatializer_info(sp, 26));
    printf("streams %d frames %lld target %.1f LUFS ceiling %.1f dBTP latency %lld: pass two clipped %llu samples\n", streams, (long long)frames,
           target_lufs, ceiling_dbtp, (long long)delay, (unsigned long long)clipped);
    for (int i = 0; i < streams; ++i)
        printf("stream %d: preset %d %.3f LUFS gain %.6f min limiter gain %.6f limited %llu of %llu frames clipped %llu\n", i, (int)which[i], ld[i].integrated_lufs,
               (double)gains[i], (double)lim[i].min_gain, (unsigned long long)lim[i].limited_frames, (unsigned long long)lim[i].frames,
               (unsigned long long)lv[i].clipped);
    if (argc > 6) {                                                   /* every stream without its first D frames: the file, aligned with the input */
        FILE *f = fopen(argv[6], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[6]); return 1; }
        for (int i = 0; i < streams; ++i)
            if (fwrite(out + ((size_t)i * (size_t)padded + (size_t)delay) * 2, sizeof(int16_t), (size_t)frames * 2, f) != (size_t)frames * 2) {
                fprintf(stderr, "cannot write %s\n", argv[6]);
                return 1;
            }
        fclose(f);
    }

    free(which);
    free(ld);
    free(lim);
    free(lv);
    free(gains);
    CHECK(aw_host_free_pinned(ctx, in));
    CHECK(aw_host_free_pinned(ctx, scratch));
    CHECK(aw_host_free_pinned(ctx, out));
    aw_spatializer_destroy(sp);
    aw_layout_destroy(layout);
    aw_context_destroy(ctx);
    return 0;
}

/* offline_batch_true_peak.c — two passes over a batch to a loudness target under a true-peak ceiling: measure both, then one gain per
 * stream, then 16-bit output.
 *
 *   N streams of interleaved 7.1 float32 in host memory  ->  HeSuVi HRIR preset  ->  N stereo s16 streams at -16 LUFS, at most -1 dBTP.
 *
 * Pass one runs the batch with the BS.1770 loudness and the true-peak measurement on and float32 output that nobody reads back in
 * full: only the per-stream records cross PCIe.  Per stream the gain is the smaller of the gain that brings it to the target loudness
 * (aw_loudness_gain) and the gain that brings its true peak to the ceiling; pass two applies them as AW_GAIN_FIXED, measures again and
 * encodes to dithered s16 on the device.  A silent stream measures -INFINITY and keeps a gain of 1.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_true_peak.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_true_peak
 *   ./offline_batch_true_peak tests/golden/hrtf/RoomSH1.0.wav [streams] [seconds] [out.s16]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>

#include "airwave_hip.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        aw_status st_ = (call);                                                                       \
        if (st_ != AW_OK) {                                                                           \
            fprintf(stderr, "%s: %s (%s)\n", #call, aw_status_string(st_), aw_last_error_message()); \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

static double dbtp(const aw_stream_true_peak *t) {
    const float p = t->true_peak[0] > t->true_peak[1] ? t->true_peak[0] : t->true_peak[1];
    return p > 0.0f ? 20.0 * log10((double)p) : -INFINITY;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s hrir.wav [streams] [seconds] [out.s16]\n", argv[0]);
        return 2;
    }
    const int streams = argc > 2 ? atoi(argv[2]) : 16;
    const double seconds = argc > 3 ? atof(argv[3]) : 2.0;
    const int64_t frames = (int64_t)(seconds * 48000.0);
    const int channels = 8;
    const double target_lufs = -16.0, ceiling_dbtp = -1.0;
    if (streams < 1 || frames < 1) return 2;

    aw_context *ctx = NULL;
    aw_layout *layout = NULL;
    aw_spatializer *sp = NULL;
    CHECK(aw_context_create(0, &ctx));
    CHECK(aw_layout_detect(channels, &layout));
    CHECK(aw_preset_activate(ctx, argv[1], 48000.0, layout, NULL, streams, &sp, NULL));
    CHECK(aw_spatializer_set_loudness(sp, 1, seconds));               /* the records are allocated now, not in process */
    CHECK(aw_spatializer_set_true_peak(sp, 1));
    CHECK(aw_spatializer_set_metering(sp, 1));                        /* the per-stream clip counts of pass two */
    CHECK(aw_spatializer_reserve_pcm(sp, frames, AW_SAMPLE_F32, AW_SAMPLE_S16));

    const size_t n_in = (size_t)streams * (size_t)frames * channels, n_out = (size_t)streams * (size_t)frames * 2;
    float *in = NULL, *scratch = NULL;
    int16_t *out = NULL;
    CHECK(aw_host_alloc_pinned(ctx, n_in * sizeof(float), (void **)&in));
    CHECK(aw_host_alloc_pinned(ctx, n_out * sizeof(float), (void **)&scratch));
    CHECK(aw_host_alloc_pinned(ctx, n_out * sizeof(int16_t), (void **)&out));
    uint32_t s = 12345u;                                              /* quiet to loud from stream to stream */
    for (size_t i = 0; i < n_in; ++i) {
        s = s * 1664525u + 1013904223u;
        in[i] = ((float)(s >> 8) / 16777216.0f - 0.5f) * (0.01f + 0.5f * (float)(i / ((size_t)frames * channels)) / (float)streams);
    }

    /* pass one: measure */
    CHECK(aw_spatializer_process_host(sp, in, scratch, frames));
    aw_stream_loudness *ld = (aw_stream_loudness *)calloc((size_t)streams, sizeof *ld);
    aw_stream_true_peak *tp = (aw_stream_true_peak *)calloc((size_t)streams, sizeof *tp);
    aw_stream_true_peak *tp2 = (aw_stream_true_peak *)calloc((size_t)streams, sizeof *tp2);
    aw_stream_levels *lv = (aw_stream_levels *)calloc((size_t)streams, sizeof *lv);
    float *gains = (float *)calloc((size_t)streams, sizeof *gains);
    if (!ld || !tp || !tp2 || !lv || !gains) return 1;
    CHECK(aw_spatializer_get_loudness(sp, 0, streams, ld));
    CHECK(aw_spatializer_get_true_peak(sp, 0, streams, tp));
    const double ceiling = pow(10.0, ceiling_dbtp / 20.0);
    for (int i = 0; i < streams; ++i) {
        if (aw_loudness_gain(ld[i].integrated_lufs, target_lufs, &gains[i]) != AW_OK) gains[i] = 1.0f;     /* silence: nothing to bring anywhere */
        const double peak = tp[i].true_peak[0] > tp[i].true_peak[1] ? tp[i].true_peak[0] : tp[i].true_peak[1];
        if (peak * (double)gains[i] > ceiling) gains[i] = (float)(ceiling / peak);
    }

    /* pass two: the same input from the start, fixed gains, dithered s16; the measurement again, now of what the gains will scale */
    CHECK(aw_spatializer_reset(sp));                                  /* also starts the measurements over */
    CHECK(aw_spatializer_set_loudness(sp, 0, 0.0));
    CHECK(aw_spatializer_set_gain(sp, AW_GAIN_FIXED, gains, streams, 0.0f));
    CHECK(aw_spatializer_set_dither(sp, AW_DITHER_TPDF, 1, 0));
    uint64_t clipped = 0;
    CHECK(aw_spatializer_process_host_pcm(sp, in, AW_SAMPLE_F32, out, AW_SAMPLE_S16, frames, &clipped));
    CHECK(aw_spatializer_get_levels(sp, 0, streams, lv));
    CHECK(aw_spatializer_get_true_peak(sp, 0, streams, tp2));
    printf("streams %d frames %lld target %.1f LUFS ceiling %.1f dBTP: pass two clipped %llu samples\n", streams, (long long)frames, target_lufs,
           ceiling_dbtp, (unsigned long long)clipped);
    for (int i = 0; i < streams; ++i)
        printf("stream %d: %.3f LUFS %.3f dBTP gain %.6f out %.3f LUFS %.3f dBTP clipped %llu\n", i, ld[i].integrated_lufs, dbtp(&tp[i]), (double)gains[i],
               ld[i].integrated_lufs + 20.0 * log10((double)gains[i]), dbtp(&tp2[i]) + 20.0 * log10((double)gains[i]),
               (unsigned long long)lv[i].clipped);
    if (argc > 4) {
        FILE *f = fopen(argv[4], "wb");
        if (!f || fwrite(out, sizeof(int16_t), n_out, f) != n_out) { fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
        fclose(f);
    }

    free(ld);
    free(tp);
    free(tp2);
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

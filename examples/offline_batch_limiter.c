/* offline_batch_limiter.c — two passes over a batch to a loudness target AND a true-peak ceiling at once: measure the loudness, then one
 * gain per stream behind a look-ahead true-peak limiter, then 16-bit output.
 *
 *   N streams of interleaved 7.1 float32 in host memory  ->  HeSuVi HRIR preset  ->  N stereo s16 streams at -16 LUFS, at most -1 dBTP.
 *
 * Pass one runs the batch with the BS.1770 loudness measurement on and float32 output that nobody reads back: only the per-stream records
 * cross PCIe.  Pass two applies the gains that bring every stream to the target (aw_loudness_gain) as AW_GAIN_FIXED, limits what then
 * exceeds the ceiling on the device (aw_spatializer_set_limiter) and encodes to dithered s16 — where offline_batch_true_peak.c has to
 * turn a whole stream down by what its single worst inter-sample peak demands.  The limiter delays its output by D frames
 * (aw_spatializer_info 24): the host feeds D frames of zeros behind the file and drops the first D output frames.  A silent stream
 * measures -INFINITY and keeps a gain of 1.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_limiter.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_limiter
 *   ./offline_batch_limiter tests/golden/hrtf/RoomSH1.0.wav [streams] [seconds] [out.s16]
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
    const int32_t attack = 64, hold = 128;
    if (streams < 1 || frames < 1) return 2;

    aw_context *ctx = NULL;
    aw_layout *layout = NULL;
    aw_spatializer *sp = NULL;
    CHECK(aw_context_create(0, &ctx));
    CHECK(aw_layout_detect(channels, &layout));
    CHECK(aw_preset_activate(ctx, argv[1], 48000.0, layout, NULL, streams, &sp, NULL));
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

    /* pass one: measure (the zeros behind the file add silence, which the gates drop) */
    CHECK(aw_spatializer_process_host(sp, in, scratch, padded));
    aw_stream_loudness *ld = (aw_stream_loudness *)calloc((size_t)streams, sizeof *ld);
    aw_stream_limiter *lim = (aw_stream_limiter *)calloc((size_t)streams, sizeof *lim);
    aw_stream_levels *lv = (aw_stream_levels *)calloc((size_t)streams, sizeof *lv);
    float *gains = (float *)calloc((size_t)streams, sizeof *gains);
    if (!ld || !lim || !lv || !gains) return 1;
    CHECK(aw_spatializer_get_loudness(sp, 0, streams, ld));
    for (int i = 0; i < streams; ++i)
        if (aw_loudness_gain(ld[i].integrated_lufs, target_lufs, &gains[i]) != AW_OK) gains[i] = 1.0f;     /* silence: nothing to bring anywhere */

    /* pass two: the same input from the start, fixed gains, the limiter, dithered s16 */
    CHECK(aw_spatializer_reset(sp));
    CHECK(aw_spatializer_set_loudness(sp, 0, 0.0));
    CHECK(aw_spatializer_set_gain(sp, AW_GAIN_FIXED, gains, streams, 0.0f));
    CHECK(aw_spatializer_set_limiter(sp, 1, (float)pow(10.0, ceiling_dbtp / 20.0), attack, hold));
    CHECK(aw_spatializer_set_dither(sp, AW_DITHER_TPDF, 1, 0));
    uint64_t clipped = 0;
    CHECK(aw_spatializer_process_host_pcm(sp, in, AW_SAMPLE_F32, out, AW_SAMPLE_S16, padded, &clipped));
    CHECK(aw_spatializer_get_levels(sp, 0, streams, lv));
    CHECK(aw_spatializer_get_limiter(sp, 0, streams, lim));
    printf("streams %d frames %lld target %.1f LUFS ceiling %.1f dBTP latency %lld: pass two clipped %llu samples\n", streams, (long long)frames,
           target_lufs, ceiling_dbtp, (long long)delay, (unsigned long long)clipped);
    for (int i = 0; i < streams; ++i)
        printf("stream %d: %.3f LUFS gain %.6f min limiter gain %.6f limited %llu of %llu frames clipped %llu\n", i, ld[i].integrated_lufs,
               (double)gains[i], (double)lim[i].min_gain, (unsigned long long)lim[i].limited_frames, (unsigned long long)lim[i].frames,
               (unsigned long long)lv[i].clipped);
    if (argc > 4) {                                                   /* every stream without its first D frames: the file, aligned with the input */
        FILE *f = fopen(argv[4], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
        for (int i = 0; i < streams; ++i)
            if (fwrite(out + ((size_t)i * (size_t)padded + (size_t)delay) * 2, sizeof(int16_t), (size_t)frames * 2, f) != (size_t)frames * 2) {
                fprintf(stderr, "cannot write %s\n", argv[4]);
                return 1;
            }
        fclose(f);
    }

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

/* offline_batch_resample_pcm.c — a mixed-rate batch of 16-bit PCM delivered as 16-bit PCM at one rate, with no float32 over PCIe: two
 * buckets of streams, at 44.1 kHz and at 96 kHz, are spatialized at their own rates and converted to 48 kHz on the device.
 *
 *   N streams of interleaved 7.1 s16 per bucket  ->  HeSuVi HRIR preset at the bucket's rate (s16 in, float32 on the device)
 *                                                ->  aw_pcm_rateconv: fixed gain, TPDF dither, metering  ->  stereo s16 at 48 kHz.
 *
 * The converter's output is the file the host delivers, so the gain, the dither, the clip count and the levels are the converter's: the
 * spatializer hands it float32 on the device, and the converter's kernel encodes s16 on its way out.  The dither's first stream is the
 * bucket's first global stream, so the batch gets the noise one handle holding every stream would give it.  The records outlive the
 * flush: they are read once, at the end.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_resample_pcm.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_resample_pcm
 *   ./offline_batch_resample_pcm tests/golden/hrtf/RoomSH1.0.wav [streams per bucket] [seconds] [gain]
 */
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

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s hrir.wav [streams per bucket] [seconds] [gain]\n", argv[0]);
        return 2;
    }
    const int streams = argc > 2 ? atoi(argv[2]) : 4;
    const double seconds = argc > 3 ? atof(argv[3]) : 1.0;
    const float gain = argc > 4 ? (float)atof(argv[4]) : 0.5f;
    const double out_rate = 48000.0, rates[2] = {44100.0, 96000.0};
    const uint64_t seed = 2024u;
    const int channels = 8;
    if (streams < 1 || !(seconds > 0.0)) return 2;

    aw_context *ctx = NULL;
    aw_layout *layout = NULL;
    CHECK(aw_context_create(0, &ctx));
    CHECK(aw_layout_detect(channels, &layout));

    for (int b = 0; b < 2; ++b) {
        const int64_t frames = (int64_t)(seconds * rates[b]);
        int32_t L = 0, M = 0, taps = 0, latency = 0;
        if (frames < 1) return 2;
        CHECK(aw_rateconv_plan(rates[b], out_rate, &L, &M, &taps, &latency));
        const int64_t total = (frames * L + M - 1) / M;                    /* what the bucket leaves with, flushed */

        aw_spatializer *sp = NULL;
        aw_rateconv *rc = NULL;
        CHECK(aw_preset_activate(ctx, argv[1], rates[b], layout, NULL, streams, &sp, NULL));
        CHECK(aw_rateconv_create(ctx, rates[b], out_rate, streams, 2, &rc));
        /* the settings of the PCM entries; each setter allocates at most once, here and never on the process path */
        CHECK(aw_pcm_rateconv_set_gain(rc, AW_GAIN_FIXED, &gain, 1));
        CHECK(aw_pcm_rateconv_set_dither(rc, AW_DITHER_TPDF, seed, (uint64_t)b * (uint64_t)streams));
        CHECK(aw_pcm_rateconv_set_metering(rc, 1));

        const size_t n_in = (size_t)streams * (size_t)frames * channels, n_mid = (size_t)streams * (size_t)frames * 2;
        const size_t n_out = (size_t)streams * (size_t)total * 2;
        int16_t *in = (int16_t *)malloc(n_in * sizeof(int16_t)), *out = (int16_t *)malloc(n_out * sizeof(int16_t));
        if (!in || !out) return 1;
        uint32_t s = 12345u + (uint32_t)b;
        for (size_t i = 0; i < n_in; ++i) {
            s = s * 1664525u + 1013904223u;
            in[i] = (int16_t)((int32_t)(s >> 18) - 8192);                  /* uniform in a quarter of full scale */
        }
        void *d_in = NULL, *d_mid = NULL, *d_head = NULL, *d_tail = NULL;
        CHECK(aw_device_alloc(ctx, n_in * sizeof(int16_t), &d_in));
        CHECK(aw_device_alloc(ctx, n_mid * sizeof(float), &d_mid));
        CHECK(aw_memcpy_h2d(ctx, d_in, in, n_in * sizeof(int16_t)));

        /* spatialize at the bucket's rate, convert, flush: three calls queued back to back */
        const int64_t head = aw_rateconv_output_frames(rc, frames);
        int64_t made = 0, rest = 0;
        CHECK(aw_device_alloc(ctx, (size_t)streams * (size_t)(head > 0 ? head : 1) * 2 * sizeof(int16_t), &d_head));
        CHECK(aw_device_alloc(ctx, (size_t)streams * (size_t)(total - head > 0 ? total - head : 1) * 2 * sizeof(int16_t), &d_tail));
        CHECK(aw_spatializer_process_pcm(sp, d_in, AW_SAMPLE_S16, d_mid, AW_SAMPLE_F32, frames, NULL));
        CHECK(aw_pcm_rateconv_process(rc, d_mid, AW_SAMPLE_F32, frames, d_head, AW_SAMPLE_S16, head, &made, NULL));
        CHECK(aw_pcm_rateconv_flush(rc, d_tail, AW_SAMPLE_S16, total - head, &rest, NULL));
        if (made != head || made + rest != total) {
            fprintf(stderr, "the converter produced %lld + %lld frames, expected %lld\n", (long long)made, (long long)rest, (long long)total);
            return 1;
        }
        /* the two calls write [streams][made][2] and [streams][rest][2] s16: stitched per stream on the way back; `out` is the file */
        int16_t *part = (int16_t *)malloc((size_t)streams * (size_t)(made > rest ? made : rest) * 2 * sizeof(int16_t));
        aw_rateconv_levels *levels = (aw_rateconv_levels *)malloc((size_t)streams * sizeof(aw_rateconv_levels));
        if (!part || !levels) return 1;
        CHECK(aw_memcpy_d2h(ctx, part, d_head, (size_t)streams * (size_t)made * 2 * sizeof(int16_t)));
        for (int i = 0; i < streams; ++i)
            for (int64_t k = 0; k < made * 2; ++k) out[(size_t)i * (size_t)total * 2 + (size_t)k] = part[(size_t)i * (size_t)made * 2 + (size_t)k];
        CHECK(aw_memcpy_d2h(ctx, part, d_tail, (size_t)streams * (size_t)rest * 2 * sizeof(int16_t)));
        for (int i = 0; i < streams; ++i)
            for (int64_t k = 0; k < rest * 2; ++k)
                out[(size_t)i * (size_t)total * 2 + (size_t)(made * 2 + k)] = part[(size_t)i * (size_t)rest * 2 + (size_t)k];
        CHECK(aw_pcm_rateconv_get_levels(rc, 0, streams, levels));          /* after the flush: the records are still there */

        printf("bucket %.0f Hz -> %.0f Hz: L %d M %d taps %d latency %d; %d streams, %lld frames in, %lld + %lld = %lld frames out\n", rates[b], out_rate,
               (int)L, (int)M, (int)taps, (int)latency, streams, (long long)frames, (long long)made, (long long)rest, (long long)total);
        for (int i = 0; i < streams; ++i) {
            int64_t rails = 0;
            for (int64_t k = 0; k < total * 2; ++k) {
                const int16_t v = out[(size_t)i * (size_t)total * 2 + (size_t)k];
                rails += v == 32767 || v == -32768;
            }
            printf("stream %d at %.0f Hz: %llu frames at %.0f Hz, peak %.9g before the gain of %.9g, clipped %llu, at the rails %lld, nonfinite %llu\n", i,
                   rates[b], (unsigned long long)levels[i].frames, out_rate, (double)levels[i].peak, (double)gain, (unsigned long long)levels[i].clipped,
                   (long long)rails, (unsigned long long)levels[i].nonfinite);
        }

        free(levels);
        free(part);
        free(in);
        free(out);
        CHECK(aw_device_free(ctx, d_in));
        CHECK(aw_device_free(ctx, d_mid));
        CHECK(aw_device_free(ctx, d_head));
        CHECK(aw_device_free(ctx, d_tail));
        aw_rateconv_destroy(rc);
        aw_spatializer_destroy(sp);
    }
    aw_layout_destroy(layout);
    aw_context_destroy(ctx);
    return 0;
}

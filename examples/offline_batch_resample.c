/* offline_batch_resample.c — a mixed-rate batch delivered at one rate: two buckets of streams, at 44.1 kHz and at 96 kHz, are spatialized
 * at their own rates and converted to 48 kHz on the device.
 *
 *   N streams of interleaved 7.1 float32 per bucket  ->  HeSuVi HRIR preset at the bucket's rate  ->  aw_rateconv  ->  stereo at 48 kHz.
 *
 * The HRIR is resampled to each bucket's rate as the reference does at activation (aw_preset_activate); the AUDIO goes through
 * aw_rateconv, a polyphase Kaiser-windowed sinc, behind the spatializer.  Everything between the upload and the download stays on the
 * device and is queued on the context's stream: process, convert, flush.  A bucket of F input frames leaves with ceil(F L / M) frames.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_resample.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_resample
 *   ./offline_batch_resample tests/golden/hrtf/RoomSH1.0.wav [streams per bucket] [seconds]
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

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s hrir.wav [streams per bucket] [seconds]\n", argv[0]);
        return 2;
    }
    const int streams = argc > 2 ? atoi(argv[2]) : 4;
    const double seconds = argc > 3 ? atof(argv[3]) : 1.0;
    const double out_rate = 48000.0, rates[2] = {44100.0, 96000.0};
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
        CHECK(aw_rateconv_create(ctx, rates[b], out_rate, streams, 2, &rc));          /* every device allocation of the converter */

        const size_t n_in = (size_t)streams * (size_t)frames * channels, n_mid = (size_t)streams * (size_t)frames * 2;
        const size_t n_out = (size_t)streams * (size_t)total * 2;
        float *in = (float *)malloc(n_in * sizeof(float)), *out = (float *)malloc(n_out * sizeof(float));
        if (!in || !out) return 1;
        uint32_t s = 12345u + (uint32_t)b;
        for (size_t i = 0; i < n_in; ++i) {
            s = s * 1664525u + 1013904223u;
            in[i] = ((float)(s >> 8) / 16777216.0f - 0.5f) * 0.25f;
        }
        void *d_in = NULL, *d_mid = NULL, *d_head = NULL, *d_tail = NULL;
        CHECK(aw_device_alloc(ctx, n_in * sizeof(float), &d_in));
        CHECK(aw_device_alloc(ctx, n_mid * sizeof(float), &d_mid));
        CHECK(aw_memcpy_h2d(ctx, d_in, in, n_in * sizeof(float)));

        /* spatialize at the bucket's rate, convert, flush: three calls queued back to back */
        const int64_t head = aw_rateconv_output_frames(rc, frames);
        int64_t made = 0, rest = 0;
        CHECK(aw_device_alloc(ctx, (size_t)streams * (size_t)(head > 0 ? head : 1) * 2 * sizeof(float), &d_head));
        CHECK(aw_device_alloc(ctx, (size_t)streams * (size_t)(total - head > 0 ? total - head : 1) * 2 * sizeof(float), &d_tail));
        CHECK(aw_spatializer_process(sp, (const float *)d_in, (float *)d_mid, frames));
        CHECK(aw_rateconv_process(rc, (const float *)d_mid, frames, (float *)d_head, head, &made));
        CHECK(aw_rateconv_flush(rc, (float *)d_tail, total - head, &rest));
        if (made != head || made + rest != total) {
            fprintf(stderr, "the converter produced %lld + %lld frames, expected %lld\n", (long long)made, (long long)rest, (long long)total);
            return 1;
        }
        /* the two calls write [streams][made][2] and [streams][rest][2]: stitched per stream on the way back */
        float *part = (float *)malloc((size_t)streams * (size_t)(made > rest ? made : rest) * 2 * sizeof(float));
        if (!part) return 1;
        CHECK(aw_memcpy_d2h(ctx, part, d_head, (size_t)streams * (size_t)made * 2 * sizeof(float)));
        for (int i = 0; i < streams; ++i)
            for (int64_t k = 0; k < made * 2; ++k) out[(size_t)i * (size_t)total * 2 + (size_t)k] = part[(size_t)i * (size_t)made * 2 + (size_t)k];
        CHECK(aw_memcpy_d2h(ctx, part, d_tail, (size_t)streams * (size_t)rest * 2 * sizeof(float)));
        for (int i = 0; i < streams; ++i)
            for (int64_t k = 0; k < rest * 2; ++k)
                out[(size_t)i * (size_t)total * 2 + (size_t)(made * 2 + k)] = part[(size_t)i * (size_t)rest * 2 + (size_t)k];

        printf("bucket %.0f Hz -> %.0f Hz: L %d M %d taps %d latency %d; %d streams, %lld frames in, %lld + %lld = %lld frames out\n", rates[b], out_rate,
               (int)L, (int)M, (int)taps, (int)latency, streams, (long long)frames, (long long)made, (long long)rest, (long long)total);
        for (int i = 0; i < streams; ++i) {
            float peak = 0.0f;
            for (int64_t k = 0; k < total * 2; ++k) {
                const float a = fabsf(out[(size_t)i * (size_t)total * 2 + (size_t)k]);
                if (!(a <= peak)) peak = a;                                 /* (a NaN would show) */
            }
            printf("stream %d at %.0f Hz: %lld frames at %.0f Hz, peak %.6f\n", i, rates[b], (long long)total, out_rate, (double)peak);
        }

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

/* offline_batch_resample_true_peak.c — a mixed-rate batch delivered as 16-bit PCM at 48 kHz under a true-peak ceiling of -1 dBTP that is
 * measured where it counts: behind the rate converter.  Resampling moves inter-sample peaks, so a ceiling held at 44.1 kHz does not hold at
 * 48 kHz; here the converter measures its own output, and no float32 crosses PCIe.
 *
 *   N streams of interleaved 7.1 s16 per bucket (44.1 kHz, 96 kHz)  ->  HeSuVi HRIR preset at the bucket's rate (float32 on the device)
 *     pass one:  aw_tp_rateconv_measure + _measure_flush            ->  the true peak of every stream at 48 kHz, nothing written
 *     host:      g = tp > c ? c / tp : 1                            ->  aw_pcm_rateconv_set_gain(AW_GAIN_FIXED)
 *     pass two:  aw_pcm_rateconv_process + _flush, TPDF dither      ->  stereo s16 at 48 kHz
 *
 * The converter's outputs are a pure function of its input, so pass two produces the samples pass one measured: its own records (measuring
 * stays on) repeat pass one's bit for bit, which the program checks.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_resample_true_peak.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_resample_true_peak
 *   ./offline_batch_resample_true_peak tests/golden/hrtf/RoomSH1.0.wav [streams per bucket] [seconds] [out.s16]
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

static double dbtp(float peak) { return peak > 0.0f ? 20.0 * log10((double)peak) : -200.0; }

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s hrir.wav [streams per bucket] [seconds] [out.s16]\n", argv[0]);
        return 2;
    }
    const int streams = argc > 2 ? atoi(argv[2]) : 4;
    const double seconds = argc > 3 ? atof(argv[3]) : 1.0;
    const char *out_path = argc > 4 ? argv[4] : NULL;
    const double out_rate = 48000.0, rates[2] = {44100.0, 96000.0};
    const float ceiling = 0.891250938f;                                    /* -1 dBTP */
    const uint64_t seed = 2024u;
    const int channels = 8;
    if (streams < 1 || !(seconds > 0.0)) return 2;

    aw_context *ctx = NULL;
    aw_layout *layout = NULL;
    CHECK(aw_context_create(0, &ctx));
    CHECK(aw_layout_detect(channels, &layout));
    FILE *file = out_path ? fopen(out_path, "wb") : NULL;
    if (out_path && !file) return 1;

    for (int b = 0; b < 2; ++b) {
        const int64_t frames = (int64_t)(seconds * rates[b]);
        int32_t L = 0, M = 0;
        if (frames < 1) return 2;
        CHECK(aw_rateconv_plan(rates[b], out_rate, &L, &M, NULL, NULL));
        const int64_t total = (frames * L + M - 1) / M;                    /* what the bucket leaves with, flushed */

        aw_spatializer *sp = NULL;
        aw_rateconv *rc = NULL;
        CHECK(aw_preset_activate(ctx, argv[1], rates[b], layout, NULL, streams, &sp, NULL));
        CHECK(aw_rateconv_create(ctx, rates[b], out_rate, streams, 2, &rc));
        CHECK(aw_tp_rateconv_set(rc, 1));                                  /* the feature's one allocation, here and never on a process path */
        CHECK(aw_pcm_rateconv_set_dither(rc, AW_DITHER_TPDF, seed, (uint64_t)b * (uint64_t)streams));

        const size_t n_in = (size_t)streams * (size_t)frames * channels, n_mid = (size_t)streams * (size_t)frames * 2;
        const size_t n_out = (size_t)streams * (size_t)total * 2;
        int16_t *in = (int16_t *)malloc(n_in * sizeof(int16_t)), *out = (int16_t *)malloc(n_out * sizeof(int16_t));
        aw_rateconv_true_peak *one = (aw_rateconv_true_peak *)malloc((size_t)streams * sizeof(aw_rateconv_true_peak));
        aw_rateconv_true_peak *two = (aw_rateconv_true_peak *)malloc((size_t)streams * sizeof(aw_rateconv_true_peak));
        float *gains = (float *)malloc((size_t)streams * sizeof(float));
        if (!in || !out || !one || !two || !gains) return 1;
        uint32_t s = 12345u + (uint32_t)b;
        for (size_t i = 0; i < n_in; ++i) {                                /* uniform noise; stream i at a quarter, an eighth, a sixteenth of full scale */
            const int stream = (int)(i / ((size_t)frames * channels));
            s = s * 1664525u + 1013904223u;
            in[i] = (int16_t)(((int32_t)(s >> 18) - 8192) / (1 << (stream % 3)));
        }
        void *d_in = NULL, *d_mid = NULL, *d_head = NULL, *d_tail = NULL, *d_clipped = NULL;
        const uint64_t zero = 0;
        CHECK(aw_device_alloc(ctx, n_in * sizeof(int16_t), &d_in));
        CHECK(aw_device_alloc(ctx, n_mid * sizeof(float), &d_mid));
        CHECK(aw_device_alloc(ctx, sizeof(uint64_t), &d_clipped));
        CHECK(aw_memcpy_h2d(ctx, d_in, in, n_in * sizeof(int16_t)));
        CHECK(aw_memcpy_h2d(ctx, d_clipped, &zero, sizeof zero));
        CHECK(aw_spatializer_process_pcm(sp, d_in, AW_SAMPLE_S16, d_mid, AW_SAMPLE_F32, frames, NULL));

        /* pass one: measure what the converter will deliver */
        int64_t seen = 0, owed = 0;
        CHECK(aw_tp_rateconv_measure(rc, d_mid, AW_SAMPLE_F32, frames, &seen));
        CHECK(aw_tp_rateconv_measure_flush(rc, &owed));
        CHECK(aw_tp_rateconv_get(rc, 0, streams, one));
        for (int i = 0; i < streams; ++i) gains[i] = one[i].true_peak > ceiling ? ceiling / one[i].true_peak : 1.0f;
        CHECK(aw_pcm_rateconv_set_gain(rc, AW_GAIN_FIXED, gains, streams));
        CHECK(aw_tp_rateconv_reset_records(rc));

        /* pass two: the same input again, gained, dithered and encoded */
        const int64_t head = aw_rateconv_output_frames(rc, frames);
        int64_t made = 0, rest = 0;
        CHECK(aw_device_alloc(ctx, (size_t)streams * (size_t)(head > 0 ? head : 1) * 2 * sizeof(int16_t), &d_head));
        CHECK(aw_device_alloc(ctx, (size_t)streams * (size_t)(total - head > 0 ? total - head : 1) * 2 * sizeof(int16_t), &d_tail));
        CHECK(aw_pcm_rateconv_process(rc, d_mid, AW_SAMPLE_F32, frames, d_head, AW_SAMPLE_S16, head, &made, (uint64_t *)d_clipped));
        CHECK(aw_pcm_rateconv_flush(rc, d_tail, AW_SAMPLE_S16, total - head, &rest, (uint64_t *)d_clipped));
        CHECK(aw_tp_rateconv_get(rc, 0, streams, two));
        if (made != seen || rest != owed || made + rest != total) {
            fprintf(stderr, "pass one saw %lld + %lld frames, pass two wrote %lld + %lld, expected %lld\n", (long long)seen, (long long)owed, (long long)made,
                    (long long)rest, (long long)total);
            return 1;
        }
        if (memcmp(one, two, (size_t)streams * sizeof(aw_rateconv_true_peak)) != 0) {
            fprintf(stderr, "pass two measured something other than pass one\n");
            return 1;
        }
        int16_t *part = (int16_t *)malloc((size_t)streams * (size_t)(made > rest ? made : rest) * 2 * sizeof(int16_t));
        uint64_t clipped = 0;
        if (!part) return 1;
        CHECK(aw_memcpy_d2h(ctx, part, d_head, (size_t)streams * (size_t)made * 2 * sizeof(int16_t)));
        for (int i = 0; i < streams; ++i)
            for (int64_t k = 0; k < made * 2; ++k) out[(size_t)i * (size_t)total * 2 + (size_t)k] = part[(size_t)i * (size_t)made * 2 + (size_t)k];
        CHECK(aw_memcpy_d2h(ctx, part, d_tail, (size_t)streams * (size_t)rest * 2 * sizeof(int16_t)));
        for (int i = 0; i < streams; ++i)
            for (int64_t k = 0; k < rest * 2; ++k)
                out[(size_t)i * (size_t)total * 2 + (size_t)(made * 2 + k)] = part[(size_t)i * (size_t)rest * 2 + (size_t)k];
        CHECK(aw_memcpy_d2h(ctx, &clipped, d_clipped, sizeof clipped));
        if (file && fwrite(out, sizeof(int16_t), n_out, file) != n_out) return 1;

        printf("bucket %.0f Hz -> %.0f Hz: %d streams, %lld frames in, %lld frames out, ceiling %.3f dBTP, clipped %llu\n", rates[b], out_rate, streams,
               (long long)frames, (long long)total, dbtp(ceiling), (unsigned long long)clipped);
        for (int i = 0; i < streams; ++i)
            printf("stream %d at %.0f Hz: %.3f dBTP before (sample peak %.3f dBFS), gain %.9g, %.3f dBTP after, %llu frames\n", i, rates[b],
                   dbtp(one[i].true_peak), dbtp(one[i].sample_peak), (double)gains[i], dbtp(gains[i] * one[i].true_peak), (unsigned long long)two[i].frames);

        free(part);
        free(gains);
        free(two);
        free(one);
        free(in);
        free(out);
        CHECK(aw_device_free(ctx, d_in));
        CHECK(aw_device_free(ctx, d_mid));
        CHECK(aw_device_free(ctx, d_head));
        CHECK(aw_device_free(ctx, d_tail));
        CHECK(aw_device_free(ctx, d_clipped));
        aw_rateconv_destroy(rc);
        aw_spatializer_destroy(sp);
    }
    if (file) fclose(file);
    aw_layout_destroy(layout);
    aw_context_destroy(ctx);
    return 0;
}

/* offline_batch_multi.c — one batch over several GPUs from a single-threaded C99 host: no RCCL, no second process, no pthreads.
 *
 *   N streams of interleaved 7.1 s16 in host memory  ->  HeSuVi HRIR preset  ->  N stereo s16 streams, gained and dithered,
 *   the streams spread over the listed devices by one aw_multi handle (the worker threads live in the library).
 *
 * The device list names one ordinal per shard; an ordinal may repeat ("0,0": two contexts on one GPU, which is how a one-GPU box runs
 * this).  Shard i owns a contiguous run of streams (aw_multi_shard).  The buffers are page-locked memory every listed device can DMA
 * (aw_multi_alloc_pinned), laid out exactly as one aw_spatializer of N streams would take them.
 *
 *   cc -std=c99 -O2 -Iinclude examples/offline_batch_multi.c -Lairwave_amd -lairwave_hip -Wl,-rpath,$PWD/airwave_amd -Wl,-rpath,/opt/rocm/lib -lm -o offline_batch_multi
 *   ./offline_batch_multi tests/golden/hrtf/RoomSH1.0.wav 0,1,2,3 [streams] [seconds] [out.s16] [repetitions]
 * repetitions: the process call is repeated from the programme's start that many times and timed each time (the first is the warm-up).
 */
#define _POSIX_C_SOURCE 199309L        /* clock_gettime under -std=c99 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <time.h>

#include "airwave_hip.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        aw_status st_ = (call);                                                                       \
        if (st_ != AW_OK) {                                                                           \
            fprintf(stderr, "%s: %s (%s)\n", #call, aw_status_string(st_), aw_last_error_message()); \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

#define SEED 20240u
#define DITHER_SEED 7u

static double now_seconds(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s hrir.wav devices(e.g. 0,0 or 0,1,2,3) [streams] [seconds] [out.s16] [repetitions]\n", argv[0]);
        return 2;
    }
    int32_t devices[64];
    int32_t n_devices = 0;
    for (const char *p = argv[2]; *p;) {
        char *end = NULL;
        const long v = strtol(p, &end, 10);
        if (end == p || (*end && *end != ',') || n_devices == 64) {
            fprintf(stderr, "devices: a comma-separated list of 1 to 64 ordinals, got \"%s\"\n", argv[2]);
            return 2;
        }
        devices[n_devices++] = (int32_t)v;
        p = *end == ',' ? end + 1 : end;
    }
    const int streams = argc > 3 ? atoi(argv[3]) : 16;
    const double seconds = argc > 4 ? atof(argv[4]) : 1.0;
    const char *out_path = argc > 5 && argv[5][0] ? argv[5] : NULL;
    const int repetitions = argc > 6 ? atoi(argv[6]) : 1;
    const int64_t frames = (int64_t)(seconds * 48000.0);
    const int channels = 8;
    if (n_devices < 1 || streams < 1 || frames < 1 || repetitions < 1) return 2;

    const int32_t visible = aw_device_count();
    if (visible < 1) {
        fprintf(stderr, "no HIP device visible (this library has no CPU fallback)\n");
        return 1;
    }
    printf("%d HIP device%s visible\n", (int)visible, visible == 1 ? "" : "s");
    for (int32_t i = 0; i < n_devices; ++i) {                         /* only the listed ones: asking opens the device */
        int seen = 0;
        for (int32_t j = 0; j < i; ++j) seen |= devices[j] == devices[i];
        if (seen) continue;
        struct aw_device_info info;
        CHECK(aw_device_info(devices[i], &info));
        printf("device %d: %s (%s), %d compute units, %.1f of %.1f GiB free\n", (int)devices[i], info.name, info.arch, (int)info.compute_units,
               (double)info.free_bytes / 1073741824.0, (double)info.total_bytes / 1073741824.0);
    }

    /* the preset: HRIR tracks from the WAV, the 7.1 layout resolved through the HeSuVi map (what aw_preset_activate does for one handle) */
    aw_wav *wav = NULL;
    aw_layout *layout = NULL;
    aw_channel_map *map = NULL;
    int32_t left[8], right[8];
    CHECK(aw_wav_load(argv[1], &wav));
    CHECK(aw_layout_detect(channels, &layout));
    if (aw_wav_channel_count(wav) == 7) CHECK(aw_map_hesuvi7(layout, &map));
    else CHECK(aw_map_hesuvi14(layout, &map));
    CHECK(aw_map_resolve(map, layout, aw_wav_channel_count(wav), left, right));

    aw_multi *m = NULL;
    CHECK(aw_multi_create(devices, n_devices, aw_wav_planar(wav), aw_wav_channel_count(wav), aw_wav_frame_count(wav), aw_wav_sample_rate(wav), channels,
                          left, right, streams, 0, &m));
    for (int32_t i = 0; i < aw_multi_shard_count(m); ++i) {
        int32_t ordinal = 0, first = 0, count = 0;
        CHECK(aw_multi_shard(m, i, &ordinal, &first, &count));
        printf("shard %d: device %d first stream %d count %d\n", (int)i, (int)ordinal, (int)first, (int)count);
    }

    const size_t n_in = (size_t)streams * (size_t)frames * (size_t)channels, n_out = (size_t)streams * (size_t)frames * 2;
    int16_t *in = NULL, *out = NULL;
    CHECK(aw_multi_alloc_pinned(m, n_in * sizeof(int16_t), (void **)&in));
    CHECK(aw_multi_alloc_pinned(m, n_out * sizeof(int16_t), (void **)&out));
    uint32_t s = SEED;                                                /* synthetic s16 input, about a quarter of full scale */
    for (size_t i = 0; i < n_in; ++i) {
        s = s * 1664525u + 1013904223u;
        in[i] = (int16_t)((int32_t)(s >> 18) - 8192);
    }
    float *gains = (float *)malloc((size_t)streams * sizeof *gains);
    if (!gains) return 1;
    for (int i = 0; i < streams; ++i) gains[i] = 0.25f + 0.5f * (float)i / (float)streams;          /* one fixed gain per stream */
    CHECK(aw_multi_set_gain(m, AW_GAIN_FIXED, gains, streams, 0.0f));
    CHECK(aw_multi_set_dither(m, AW_DITHER_TPDF, DITHER_SEED, 0));
    CHECK(aw_multi_reserve_pcm(m, frames, AW_SAMPLE_S16, AW_SAMPLE_S16));

    uint64_t clipped = 0;
    for (int r = 0; r < repetitions; ++r) {                           /* every repetition renders the same programme from its start */
        if (r > 0) CHECK(aw_multi_reset(m));
        const double t0 = now_seconds();
        CHECK(aw_multi_process_host_pcm(m, in, AW_SAMPLE_S16, out, AW_SAMPLE_S16, frames, &clipped));
        const double dt = now_seconds() - t0;
        printf("streams %d frames %lld: %.3f M stereo frames/s (%.1f ms), clipped %llu\n", streams, (long long)frames,
               (double)streams * (double)frames / dt / 1e6, dt * 1e3, (unsigned long long)clipped);
    }

    if (out_path) {
        FILE *f = fopen(out_path, "wb");
        if (!f || fwrite(out, sizeof(int16_t), n_out, f) != n_out) {
            fprintf(stderr, "cannot write %s\n", out_path);
            return 1;
        }
        fclose(f);
    }
    free(gains);
    CHECK(aw_multi_free_pinned(m, in));
    CHECK(aw_multi_free_pinned(m, out));
    aw_multi_destroy(m);
    aw_map_destroy(map);
    aw_layout_destroy(layout);
    aw_wav_destroy(wav);
    return 0;
}

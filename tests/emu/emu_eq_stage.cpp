// emu_eq_stage.cpp — TEST-ONLY: the device functions of the batch entries' equalizer stage (airwave_amd/csrc/device/eq_cascade.hpp:
// eq_stage_stream / eq_stage_sequential, the code hipcc compiles) under the CPU thread emulation of emu_ctx.hpp: one emulated workgroup
// of kEqThreads per stream (or per stream and ear) for the chunk-aligned part, eq_stage_sequential for the tail — the split the runtime
// makes.  The image behind the state (map, headers, tables) is built as aw_spatializer_set_equalizer builds it, with the library's own
// awh::eq_prepare.
#include "emu_ctx.hpp"

namespace {

struct Prepared {
    std::vector<awh::EqPrepared> prep;
    std::vector<awk::EqStagePreset> headers;
    std::vector<double> tables;
    int kmax = 0;
};

// preamps_db: [n_presets]; counts: [n_presets] filters of each; filters: [sum counts][4] = type, fc, gain, q
int prepare(double sample_rate, const double *preamps_db, const int *counts, const double *filters, int n_presets, Prepared &out) {
    out.prep.resize((size_t)n_presets);
    out.headers.resize((size_t)n_presets);
    for (int i = 0, at = 0; i < n_presets; at += counts[i], ++i) {
        awh::EqDefinition def;
        def.preamp_db = preamps_db[i];
        for (int k = 0; k < counts[i]; ++k) {
            const double *f = filters + (size_t)(at + k) * 4;
            awh::EqFilter fl;
            fl.type = (int)f[0]; fl.frequency_hz = f[1]; fl.gain_db = f[2]; fl.q = f[3];
            def.filters.push_back(fl);
        }
        int bi = 0, bk = 0;
        const int rc = awh::eq_prepare(&def, sample_rate, out.prep[(size_t)i], &bi, &bk);
        if (rc) return -rc;
        const awh::EqPrepared &q = out.prep[(size_t)i];
        awk::EqStagePreset &h = out.headers[(size_t)i];
        h.preamp = q.preamp; h.n_filters = q.n_filters; h.reserved = 0;
        h.tab_off = (long long)out.tables.size(); h.plane_off = h.tab_off + (long long)q.tab.size();
        out.tables.insert(out.tables.end(), q.tab.begin(), q.tab.end());
        out.tables.insert(out.tables.end(), q.plane.begin(), q.plane.end());
        out.kmax = std::max(out.kmax, q.n_filters);
    }
    return 0;
}

}  // namespace

extern "C" {

// y: [stream][frames][2], equalized in place; z: [stream][kmax][4], carried in and out; map: [stream] preset or -1.  kmax: the rows of z
// the caller laid out (checked against the presets').  Returns 0, a negative prepare error, or -100 for a kmax that does not match.
int emu_eq_stage(float *y, double *z, const int *map, int n_streams, long long frames, double sample_rate, const double *preamps_db,
                 const int *counts, const double *filters, int n_presets, int kmax, int ear_split) {
    using namespace awk;
    Prepared pr;
    const int rc = prepare(sample_rate, preamps_db, counts, filters, n_presets, pr);
    if (rc) return rc;
    if (kmax != pr.kmax) return -100;
    EqStageParams p{};
    p.z = z; p.map = map; p.presets = pr.headers.data(); p.tables = pr.tables.data();
    p.stride_frames = frames; p.kmax = kmax;
    const long long body = frames - frames % kEqChunk;
    if (body > 0) {
        p.y = y; p.frames = body;
        EmuShared sh(kEqThreads, (size_t)kEqLdsBytes / sizeof(cf));
        for (int s = 0; s < n_streams; ++s)
            for (int ear = 0; ear < (ear_split ? 2 : 1); ++ear)          // E = 1: one emulated workgroup per (stream, ear)
                emu_workgroup(kEqThreads, [&](int t) {
                    EmuCtx ctx{t, &sh};
                    if (ear_split) eq_stage_stream<EmuCtx, 1>(ctx, p, p.map, p.presets, p.tables, s, ear);
                    else eq_stage_stream<EmuCtx, 2>(ctx, p, p.map, p.presets, p.tables, s, 0);
                });
    }
    if (frames > body) {
        p.y = y + body * 2; p.frames = frames - body;
        for (int s = 0; s < n_streams; ++s)
            for (int ear = 0; ear < 2; ++ear) eq_stage_sequential(p, s, ear);
    }
    return 0;
}

// The plain cascade of ONE preset over every stream (eq_cascade_stream + eq_sequential on the dense [stream][K][4] state): what a stream of
// the stage must equal bit for bit.  Returns K or a negative prepare error.
int emu_eq_plain(float *y, double *z, int n_streams, long long frames, double sample_rate, double preamp_db, const double *filters, int n_filters,
                 int ear_split) {
    using namespace awk;
    Prepared pr;
    const int rc = prepare(sample_rate, &preamp_db, &n_filters, filters, 1, pr);
    if (rc) return rc;
    EqParams p{};
    p.in = y; p.out = y; p.z = z;
    p.t.tab = pr.prep[0].tab.data(); p.t.plane = pr.prep[0].plane.data();
    p.t.preamp = pr.prep[0].preamp; p.t.n_filters = pr.prep[0].n_filters;
    p.stride_frames = frames;
    const long long body = frames - frames % kEqChunk;
    if (body > 0) {
        p.frames = body;
        EmuShared sh(kEqThreads, (size_t)kEqLdsBytes / sizeof(cf));
        for (int s = 0; s < n_streams; ++s)
            for (int ear = 0; ear < (ear_split ? 2 : 1); ++ear)
                emu_workgroup(kEqThreads, [&](int t) {
                    EmuCtx ctx{t, &sh};
                    if (ear_split) eq_cascade_stream<EmuCtx, 1>(ctx, p, s, ear);
                    else eq_cascade_stream<EmuCtx, 2>(ctx, p, s, 0);
                });
    }
    if (frames > body) {
        p.in = y + body * 2; p.out = y + body * 2; p.frames = frames - body;
        for (int s = 0; s < n_streams; ++s)
            for (int ear = 0; ear < 2; ++ear) eq_sequential(p, s, ear);
    }
    return pr.prep[0].n_filters;
}

}  // extern "C"

// stage_records.hpp — where the per-stream records of the batch entries' output stages lie in each stage's ONE device allocation.  Host
// only, no HIP.  A layout declares its fields once, in order, each taking its bytes from the running offset `c`; offsets, the total and the
// range a reset zeroes follow from that list (tests/test_stage_records_host.py holds them to arithmetic written out by hand).
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>

#include "../device/eq_stage.hpp"
#include "../device/levels.hpp"
#include "../device/limiter.hpp"
#include "../device/loudness.hpp"

namespace awst {

// `per_stream` elements of T for each stream, from byte `off` of the allocation on; a ping-pong field has two such slots back to back
template <class T> struct Field {
    size_t off = 0, per_stream = 0, slot_elems = 0;
    T *at(unsigned char *base, size_t stream = 0, int slot = 0) const { return reinterpret_cast<T *>(base + off) + (size_t)slot * slot_elems + stream * per_stream; }
    size_t bytes() const { return slot_elems * sizeof(T); }                   // of one slot, every stream
};

struct Cursor {
    size_t n_streams, off = 0;
    template <class T> Field<T> take(size_t per_stream = 1, size_t slots = 1) {
        assert(off % alignof(T) == 0);
        const Field<T> f{off, per_stream, n_streams * per_stream};
        off += slots * f.bytes();
        return f;
    }
    // n elements of T that the streams share (tables, headers), on the next multiple of alignof(T)
    template <class T> Field<T> take_shared(size_t n) {
        off = (off + alignof(T) - 1) / alignof(T) * alignof(T);
        const Field<T> f{off, 0, 0};
        off += n * sizeof(T);
        return f;
    }
};

struct Equalizer {                            // Equalizer{{n_streams}, n_presets, kmax, table_doubles}; rules: device/eq_stage.hpp
    Cursor c;
    size_t n_presets, kmax, table_doubles;
    Field<double> state = c.take<double>(kmax * 4);                           // [kmax][4] per stream: a stream uses the rows of its own preset
    size_t reset_bytes = c.off;                                               // a reset zeroes the filter state; the presets stay
    Field<int32_t> map = c.take<int32_t>();                                   // the stream's preset, -1 = not equalized
    Field<awk::EqStagePreset> presets = c.take_shared<awk::EqStagePreset>(n_presets);      // one header per preset (8-byte aligned behind the map)
    Field<double> tables = c.take_shared<double>(table_doubles);             // every preset's tab, then its plane
    size_t total = c.off;
};

struct EqualizerFade {                        // EqualizerFade{{n_streams}, kmax}; rules: device/eq_stage.hpp (a target change); kmax: Equalizer's
    Cursor c;
    size_t kmax;
    Field<double> state_to = c.take<double>(kmax * 4);                        // the second bank: the state of the presets faded to, rows as Equalizer::state
    size_t reset_bytes = c.off;                                               // a reset zeroes it with the first bank; the maps stay
    Field<int32_t> to_map = c.take<int32_t>();                                // the running fade: the preset faded to, -1 = unity, kEqKeep = not fading
    Field<int32_t> pending_map = c.take<int32_t>();                           // the published target that has not begun, likewise
    size_t total = c.off;
};

struct Levels {                               // Levels{{n_streams}}; rules: device/levels.hpp
    Cursor c;
    Field<awl::Record> records = c.take<awl::Record>();
    Field<uint32_t> call_peaks = c.take<uint32_t>();                          // zeroed at the start of every call that runs the levels kernel
    size_t reset_bytes = c.off;                                               // a reset zeroes [0, reset_bytes): the FIXED gains stay
    Field<float> gains = c.take<float>();
    size_t total = c.off;
};

struct Loudness {                             // Loudness{{n_streams}, loud_cap, table_doubles}; rules: device/loudness.hpp
    Cursor c;
    size_t loud_cap, table_doubles;
    Field<double> state = c.take<double>((size_t)awlo::kFilters * 4);
    Field<unsigned long long> nonfinite = c.take<unsigned long long>();
    Field<double> hops = c.take<double>(loud_cap);
    size_t reset_bytes = c.off;                                               // a reset zeroes everything per stream
    Field<double> tables{c.off, 0, 0};                                        // the K-weighting sections' kernel tables, shared by the streams
    size_t total = c.off + table_doubles * sizeof(double);
};

struct TruePeak {                             // TruePeak{{n_streams}}; rules: device/truepeak.hpp
    Cursor c;
    Field<unsigned long long> nonfinite = c.take<unsigned long long>();
    Field<uint32_t> peaks = c.take<uint32_t>(2);
    Field<uint32_t> call_peaks = c.take<uint32_t>();                          // zeroed at the start of every call that runs the kernel
    Field<float> history = c.take<float>(2 * (size_t)awtp::kHistory, 2);      // [kHistory][2] per stream: a call reads slot cur and writes the other
    size_t total = c.off, reset_bytes = total;                                // a reset zeroes all of it
};

struct Limiter {                              // Limiter{{n_streams}, attack, hold}; rules: device/limiter.hpp
    Cursor c;
    int attack, hold;
    Field<unsigned long long> limited = c.take<unsigned long long>(), nonfinite = c.take<unsigned long long>();
    size_t reset_bytes = c.off;                                               // a reset zeroes the two counters, sets the lowest gains to 1
    Field<uint32_t> min_gain = c.take<uint32_t>();                            // and zeroes the history
    size_t hist_floats = 2 * (size_t)awlim::halo(attack, hold);               // raw u, per stream and slot
    Field<float> history = c.take<float>(hist_floats, 2);
    size_t total = c.off;
};

}  // namespace awst

"""TEST-ONLY: the cases that test_spectral_ref.py (tone levels), test_emu_spectral.py and test_gpu_spectral.py share — which kernel family, how
many channels, which HRIR length, which bin.  Plain data and the input builders; no fixtures, nothing that calls the code under test."""
from collections import namedtuple

import numpy as np

import spectral_ref as sr

# family -> transform length N of the tone bins, HRIR taps of the noise and tone cases, Welch segment L of band_rel_error
# emu_frames: frames of an emulated tone call, the shortest call any tone case of the family runs (the GPU calls are longer)
Family = namedtuple("Family", "N taps L emu_frames")
FAMILIES = {
    "ols8192": Family(8192, 4320, 8192, 9000),          # tile_ols.hpp
    "ols16384": Family(16384, 4320, 8192, 16500),       # tile_ols2.hpp: 8192-point transforms of the even / odd half-rate streams of a 16384-frame window
    "ola": Family(8192, 4320, 8192, 9000),              # tile_ola.hpp, H = 7
    "part": Family(8192, 9000, 8192, 9000),             # partitioned delay line, 3 partitions of 4096
    "lw32": Family(32 * 4096, 20000, 65536, 100000),    # tile_lw.hpp / tile_lw16.hpp: odd-frequency transforms of R x 4096 points
    "lw40": Family(40 * 4096, 20000, 65536, 30000),
    "lw128": Family(128 * 4096, 20000, 65536, 20000),
}


def tile_bins(N):
    """Around the radix-16 x 512 factorisation (k = k1 + 16 k2) and the self-paired bins 0 and N/2, which the marched CMAC gives slots of their own."""
    return [0, 1, 15, 16, 511, 512, 513, N // 2 - 1, N // 2]


def lw_bins(R):
    """(bin, half): around the rows (k = ra + R k2) and the 4096-point row transform, each also at the half-bin offset — the long-window transform is
    sampled at k + 1/2."""
    N = R * 4096
    return [(k, half) for k in (0, 1, R - 1, R, 4095, 4096, N // 2 - 1, N // 2) for half in (False, True)]


def family_bins(family):
    if family.startswith("lw"):
        return lw_bins(int(family[2:]))
    return [(k, False) for k in tile_bins(FAMILIES[family].N)]


Tone = namedtuple("Tone", "family channels k half seed")

def tone(family, channels, k, half=False):
    """The HRIR seed goes with the layout.  A case whose tone lands in a null of its direct_hrir's response (reference peak under 0.2 of the input
    amplitude, test_spectral_ref.py::test_every_tone_comes_out_at_a_usable_level) gets another seed; the bound stays."""
    return Tone(family, channels, k, half, 100 + channels)


# the thread emulation runs every bin on the narrowest layout of each kernel (its cost goes with the channel pairs); the overlap-add tile on a narrow and
# on a wide kernel
EMU_TONE_LAYOUTS = {"ols8192": [3, 10], "ols16384": [2], "ola": [8, 14], "part": [3, 2], "lw32": [1, 2], "lw40": [1], "lw128": [2]}
GPU_CHANNELS = [2, 7, 8, 14]               # odd: the folded real last channel; 14: the wide kernels
GPU_OLA_CHANNELS = [7, 8, 14]              # the library carries no stereo overlap-add tile (ola_inst.hpp)


def emu_tones(family):
    return [tone(family, c, k, half) for c in EMU_TONE_LAYOUTS[family] for k, half in family_bins(family)]


def gpu_tones(family):
    """Every bin on every layout."""
    return [tone(family, c, k, half) for c in (GPU_OLA_CHANNELS if family == "ola" else GPU_CHANNELS) for k, half in family_bins(family)]


def all_tones():
    seen = []
    for f in FAMILIES:
        for t in emu_tones(f) + gpu_tones(f):
            if t not in seen:
                seen.append(t)
    return seen


_direct = {}      # (taps, seed) -> direct_hrir, built once and kept unchanged


def tone_input(oracle, t, streams, frames):
    """(hrir, left, right, x [streams][frames][channels]) of a tone case: direct_hrir, every channel of every stream with phases of its own.  Stream s
    is the same whatever `streams` is."""
    fam = FAMILIES[t.family]
    if (fam.taps, t.seed) not in _direct:
        _direct[fam.taps, t.seed] = sr.direct_hrir(oracle, 14, fam.taps, t.seed)
        _direct[fam.taps, t.seed].setflags(write=False)
    h = _direct[fam.taps, t.seed]
    lt, rt = sr.maps(t.channels)
    flat = sr.tones(frames, streams * t.channels, fam.N, [t.k], t.half)
    x = np.ascontiguousarray(flat.reshape(frames, streams, t.channels).transpose(1, 0, 2))
    return h, lt, rt, x


def tone_id(t, kernel=None):
    return f"{kernel or t.family}-{t.channels}ch-bin{t.k}{'.5' if t.half else ''}"


# End-heavy HRIRs at the tap counts each kernel owns: the last length a window / block / partition count holds and the first of the next
END_HEAVY_TAPS = {
    "ols8192": [4320, 6145],                # 6145: the longest HRIR of an 8192-frame window (hop 2048)
    "ols16384": [6146, 12288],              # 12288: the longest of a 16384-frame window (hop 4096)
    "ola": [4097, 4609, 5121],              # the longest of blocks of H = 8, 7, 6 rows
    "part": [8192, 8193, 12288, 12289, 32768, 32769, 40961],      # 2 | 3, 3 | 4, 8 | 9 partitions; 11: a second, partial pass of the CMAC kernels
    "lw": [20480, 20481, 32768, 32769],     # history of 5 | 6 and 8 | 9 partitions
}


def end_heavy_input(oracle, channels, taps, streams, frames):
    h = sr.end_heavy_hrir(oracle, 14, taps, seed=taps)
    lt, rt = sr.maps(channels)
    return h, lt, rt, oracle.synth_input(streams, frames, channels, seed=channels)


def noise_input(oracle, family, channels, streams, frames, taps=None):
    taps = FAMILIES[family].taps if taps is None else taps
    h = oracle.synth_hrir(14, taps, seed=taps)
    lt, rt = sr.maps(channels)
    return h, lt, rt, oracle.synth_input(streams, frames, channels, seed=channels)

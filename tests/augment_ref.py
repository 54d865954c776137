"""Restatement of reverberation and additive noise (csrc/augment.hip) in numpy, float64 and float32, the inputs
of their tests and the allowances.

Reverberation of x[0 .. N) by an RIR h[0 .. L) with direct-path index d:  y[n] = sum_k h[k] x[n + d - k], n in [0, N), x zero
outside [0, N) - the full convolution read from index d on, so the output is not delayed.  Additive noise:  z[n] = y[n] + g
v[n], v[n] = clip[(start + n) mod len], g = 10^(-snr_db / 20) sqrt(P_y / P_v), the powers over the same N samples; g = 0 when
either is 0.  Bank preparation: d = the first index of max |h|, the RIR cut to [d - pre, d - pre + max_taps), pre = min(d, 32),
then scaled to unit energy in float64 and rounded to fp32.

Allowances (derived, not measured):
  convolution  |got - ref64| <= (L + 2) 2^-24 sum_k |h[k]| |x[n + d - k]|: one unit per step of an fp32 sum in any order,
               fused or not, and two to spare - the resampler's convention (tests/resample_ref.py)
  gain         |g - g64| <= 4 2^-24 g64: the host's fp32 scale (half a unit), the rounding of g (half a unit), room for the
               float64 sums' order
  mix          |z - z64| <= 4 2^-24 (|y| + |g v|): the gain's own error on g v (the two half units above, and the sums'
               order), the product's and the sum's rounding (half a unit of |y| + |g v| each, one if fused), two to spare
The float64 gain and mix references are computed from the float32 y the device was given."""
import numpy as np

U = 2.0 ** -24
PRE = 32


# ------------------------------------------------------------------------------------------------ bank preparation
def prepare_rir(h, max_taps=4096, pre=PRE, normalize=True):
    """-> (taps float32, d after the cut)"""
    h = np.asarray(h, dtype=np.float64)
    d = int(np.flatnonzero(np.abs(h) == np.abs(h).max())[0])
    p = min(d, pre)
    h = h[d - p:d - p + max_taps]
    if normalize:
        h = h / np.sqrt(np.sum(h * h))
    return h.astype(np.float32), p


# ------------------------------------------------------------------------------------------------ reverberation
def reverb(x, h, d, dtype=np.float64):
    """-> (y [N] of `dtype`, mag float64 = sum_k |h[k]| |x[n + d - k]|).  h: the fp32 taps the device reads.  float32: one
    running fp32 sum per output over k ascending."""
    x64, h64 = np.asarray(x).astype(np.float64), np.asarray(h).astype(np.float64)
    N, L = len(x64), len(h64)
    mag = np.concatenate([np.convolve(np.abs(x64), np.abs(h64)), np.zeros(N)])[d:d + N]
    if dtype == np.float64:
        return np.concatenate([np.convolve(x64, h64), np.zeros(N)])[d:d + N], mag
    # x[n + d - k] for n in [0, N): a slice of x padded by L zeros in front and L + d behind
    pad = np.concatenate([np.zeros(L, np.float32), np.asarray(x).astype(np.float32), np.zeros(L + d, np.float32)])
    h32 = np.asarray(h, dtype=np.float32)
    acc = np.zeros(N, dtype=np.float32)
    for k in range(L):
        acc = acc + h32[k] * pad[L + d - k:L + d - k + N]
    return acc, mag


def reverb_allowance(mag, taps):
    return (taps + 2) * U * mag


# ------------------------------------------------------------------------------------------------ additive noise
def noise_of(clip, start, n):
    clip = np.asarray(clip)
    return clip[(int(start) + np.arange(n)) % len(clip)]


def snr_scale(snr_db):
    """What the host hands to the device: 10^(-snr_db / 20) as one float32."""
    return np.float32(10.0 ** (-float(snr_db) / 20.0))


def mix(y, clip, start, snr_db, dtype=np.float64):
    """y: the float32 samples the device was given -> (z of `dtype`, g, |y| + |g v| in float64).  float64: the exact scale;
    float32: the fp32 scale, float64 power sums, g rounded once, then fp32 product and sum."""
    y32 = np.asarray(y).astype(np.float32)
    v32 = noise_of(clip, start, len(y32)).astype(np.float32)
    y64, v64 = y32.astype(np.float64), v32.astype(np.float64)
    py, pv = float(np.sum(y64 * y64)), float(np.sum(v64 * v64))
    ok = py > 0 and pv > 0
    if dtype == np.float64:
        g = 10.0 ** (-float(snr_db) / 20.0) * np.sqrt(py / pv) if ok else 0.0
        return y64 + g * v64, g, np.abs(y64) + np.abs(g * v64)
    g = np.float32(float(snr_scale(snr_db)) * np.sqrt(py / pv)) if ok else np.float32(0)
    return y32 + g * v32, g, np.abs(y64) + np.abs(float(g) * v64)


GAIN_ALLOWANCE = 4 * U


def mix_allowance(mag):
    return 4 * U * mag


def achieved_snr_db(y, z):
    y64, z64 = np.asarray(y).astype(np.float64), np.asarray(z).astype(np.float64)
    return 10.0 * np.log10(np.sum(y64 * y64) / np.sum((z64 - y64) ** 2))


# ------------------------------------------------------------------------------------------------ the case tables
def _speech(rs, n, scale=3000.0):
    return np.clip(np.round(rs.randn(n) * scale), -32768, 32767).astype(np.int16)


def rir_with(rs, taps, d):
    """A decaying RIR of `taps` entries whose largest magnitude sits at d (and only there)."""
    h = rs.randn(taps) * 0.2 * np.exp(-np.arange(taps) / max(taps / 4.0, 1.0))
    h = np.clip(h, -0.5, 0.5)
    h[d] = 1.0
    return h


def reverb_cases(tile, chunk, max_taps):
    """-> [(name, [int16 utterance], [RIR float64], [RIR index per row or -1])]: every launch of the convolution parity
    tests.  The RIRs are handed to the plan with pre = taps (no head cut), so d is where rir_with put it."""
    rs = np.random.RandomState(17)
    out = []
    # every RIR length of the issue, and the lengths around the kernel's tap chunk, with d at 0, in the middle and at L - 1;
    # utterances of 1500 samples: more than one wave's 1024 outputs
    rirs = []
    for taps in (1, 2, 31, 32, 33, 63, 65, 1000):
        for d in sorted({0, taps // 2, taps - 1}):
            rirs.append(rir_with(rs, taps, d))
    for taps in (chunk, chunk + 1, chunk + 63):
        rirs.append(rir_with(rs, taps, taps // 2))
    out.append(("lengths", [_speech(rs, 1500) for _ in rirs], rirs, list(range(len(rirs)))))
    out.append(("max_taps", [_speech(rs, 3000)], [rir_with(rs, max_taps, max_taps // 2 - 96)], [0]))
    edge = [rir_with(rs, 65, 20), rir_with(rs, 200, 199)]
    lens = [tile - 1, tile, 2 * tile + 1, 1023, 1024, 1025]
    out.append(("tile_edges", [_speech(rs, n) for n in lens], edge, [0, 1, 0, 1, 0, 1]))
    out.append(("shorter_than_rir", [_speech(rs, 10), _speech(rs, 1), _speech(rs, 999)],
                [rir_with(rs, 1000, 500), rir_with(rs, 1000, 999), rir_with(rs, 1000, 0)], [0, 1, 2]))
    out.append(("batch_of_one", [_speech(rs, 3001)], [rir_with(rs, 33, 7)], [0]))
    out.append(("mixed_rows", [_speech(rs, n) for n in (700, 4500, 33, 1200, 5)], [rir_with(rs, 300, 40), rir_with(rs, 64, 3)],
                [-1, 0, 1, -1, 1]))
    noise = [rs.randint(-32768, 32768, 2500).astype(np.int16) for _ in range(2)]
    out.append(("full_scale", noise, [rir_with(rs, 500, 100)], [0, 0]))
    return out


def mix_cases(tile):
    """-> [(name, [int16 utterance], [clip float32], [clip index or -1], [start], [snr_db])]"""
    rs = np.random.RandomState(23)
    clips = [(rs.randn(700) * 500).astype(np.float32),           # shorter than the utterances: wraps several times
             (rs.randn(20000) * 2000).astype(np.float32),        # longer
             (rs.randn(3000) * 50).astype(np.float32),
             np.asarray([1234.0], dtype=np.float32)]             # one sample
    utts = [_speech(rs, n) for n in (2 * tile + 809, 5000, tile + 1, tile, 900, 2000)]
    cidx = [0, 1, 2, 3, -1, 1]
    start = [123, 17000, 2999, 0, 0, 19999]                      # 2999, 19999: one sample before the clip's end
    snr = [5.0, 20.0, 12.5, 0.0, 10.0, 7.25]
    return [("mix", utts, clips, cidx, start, snr)]

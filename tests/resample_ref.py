"""Restatement of the speed-perturbation resampler (csrc/resample.hip) in numpy, float64 and float32, and the
inputs of its tests.

A speed factor s at sample rate sr resamples from orig = round(s sr) to new = sr, both over their gcd; the bank is the usual
Hann-windowed sinc polyphase bank with lpw = 6 and rolloff = 0.99; output i new + j of x[0 .. n) is sum_k h[j][k] x[i orig + k -
width] with x zero outside [0, n); ceil(new n / orig) outputs."""
import math

import numpy as np

LPW, ROLLOFF = 6, 0.99
U = 2.0 ** -24
FACTORS = [0.9, 1.0, 1.1, 0.95]          # the plan of the GPU tests, in this order
SAMPLE_RATE = 16000


def ratio(factor, sample_rate=SAMPLE_RATE):
    orig, new = int(round(factor * sample_rate)), int(sample_rate)
    g = math.gcd(orig, new)
    return orig // g, new // g


def bank(orig, new):
    """-> (width, h float64 [new, taps])"""
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(LPW * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    t = (-np.arange(new, dtype=np.float64)[:, None] / new + idx[None, :]) * base
    t = np.clip(t, -LPW, LPW)
    window = np.cos(t * np.pi / LPW / 2) ** 2
    t = t * np.pi
    h = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)
    return width, h


def out_samples(n, orig, new):
    return -(-new * int(n) // orig)


def resample(x, orig, new, dtype=np.float64):
    """-> (y [ceil(new n / orig)] of `dtype`, mag float64 = sum_k |h[j][k]| |x[..]| per output, taps).  float32: the taps
    rounded to fp32 once, a running fp32 sum over k ascending.  orig == new == 1 is the copy."""
    x = np.asarray(x)
    n = len(x)
    width, h = bank(orig, new)
    taps = h.shape[1]
    n_out = out_samples(n, orig, new)
    if orig == 1 and new == 1:
        return x.astype(dtype), np.abs(x.astype(np.float64)), taps
    o = np.arange(n_out)
    i, j = o // new, o % new
    pad = np.concatenate([np.zeros(width), x.astype(np.float64), np.zeros(width + orig + taps)])
    win = pad[(i * orig)[:, None] + np.arange(taps)[None, :]]          # x[i orig + k - width], zero outside
    hj = h[j]
    mag = (np.abs(hj) * np.abs(win)).sum(axis=1)
    if dtype == np.float64:
        return (hj * win).sum(axis=1), mag, taps
    h32, w32 = hj.astype(np.float32), win.astype(np.float32)
    acc = np.zeros(n_out, dtype=np.float32)
    for k in range(taps):
        acc = acc + h32[:, k] * w32[:, k]
    return acc, mag, taps


def allowance(mag, taps):
    """|err| <= (taps + 2) 2^-24 sum_k |h[j][k]| |x[..]|: one unit for the taps' rounding to fp32, one per step of the running
    sum (in any order, fused or not), one to spare."""
    return (taps + 2) * U * mag


def count_for_output(n_out, orig, new):
    """The sample count whose output length is n_out (None where no count gives it)."""
    n = n_out * orig // new
    for c in (n - 1, n, n + 1):
        if c > 0 and out_samples(c, orig, new) == n_out:
            return c
    return None


def cases(tile):
    """-> [(name, [int16 utterance], [index into FACTORS])]: every launch of the parity tests."""
    rs = np.random.RandomState(11)

    def speech(n, scale=3000.0):
        return np.clip(np.round(rs.randn(n) * scale), -32768, 32767).astype(np.int16)
    out = []
    # every count against every factor, in ONE launch of mixed factors: shorter than the taps (23), than the width (7)
    counts = [1, 7, 23, 400, 3001]
    rows = [(speech(n), f) for f in range(len(FACTORS)) for n in counts]
    out.append(("mixed", [r[0] for r in rows], [r[1] for r in rows]))
    orig, new = ratio(0.9)
    edge = [count_for_output(L, orig, new) for L in (tile - 1, tile, 2 * tile + 1)]
    assert None not in edge, edge
    out.append(("tile_edges", [speech(n) for n in edge], [0, 0, 0]))
    noise = [rs.randint(-32768, 32768, 3001).astype(np.int16) for _ in range(3)]
    out.append(("full_scale_noise", noise, [0, 2, 3]))
    low, high = np.full(400, -32768, np.int16), np.full(401, 32767, np.int16)
    out.append(("neighbours", [low, high, low.copy()], [2, 0, 3]))
    out.append(("batch_of_one", [speech(3001)], [2]))
    return out

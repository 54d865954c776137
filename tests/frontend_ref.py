"""A numpy restatement of the front end (include/asr_hip.h) for the tests: Kaldi-convention filterbank energies
(dither off, snip-edges), per-utterance CMVN statistics, and the finish pass (CMVN, add-deltas, SpecAugment masks, zero
padding).  `dtype=np.float64` is the truth; `dtype=np.float32` is a genuinely single-precision run of the same steps (its
error against float64 sizes the tests' allowances).  It computes its own tables and imports nothing of the product."""
import numpy as np
import scipy.fft

FLT_EPSILON = float(np.finfo(np.float32).eps)


def num_frames(n, L=400, S=160):
    return 1 + (n - L) // S if n >= L else 0


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def povey_window(L):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / (L - 1))) ** 0.85


def mel_weights(n_mels, n_fft, sample_rate, low_freq, high_freq):
    """float64 [n_mels, n_fft / 2]: triangles in mel space over FFT bins 0 .. n_fft/2 - 1 (no Nyquist bin)."""
    lo, hi = mel(low_freq), mel(high_freq)
    pts = lo + (hi - lo) * np.arange(n_mels + 2) / (n_mels + 1)
    m = mel(np.arange(n_fft // 2) * (sample_rate / float(n_fft)))
    W = np.zeros((n_mels, n_fft // 2))
    for j in range(n_mels):
        left, centre, right = pts[j], pts[j + 1], pts[j + 2]
        inside = (m > left) & (m < right)
        W[j] = np.where(inside, np.where(m <= centre, (m - left) / (centre - left), (right - m) / (right - centre)), 0.0)
    return W


def frames_of(x, L, S):
    T = num_frames(len(x), L, S)
    idx = np.arange(T)[:, None] * S + np.arange(L)[None, :]
    return x[idx] if T else np.zeros((0, L), x.dtype)


def fbank(x, dtype=np.float64, sample_rate=16000, L=400, S=160, n_fft=512, n_mels=80, low_freq=20.0, high_freq=None,
          preemph=0.97, use_log=True):
    """One utterance (1-D samples in int16 range) -> [T, n_mels] in `dtype`; every step is carried out in `dtype`."""
    high_freq = 0.5 * sample_rate if high_freq is None else high_freq
    fr = frames_of(np.asarray(x).astype(dtype), L, S)
    if fr.shape[0] == 0:
        return np.zeros((0, n_mels), dtype)
    c = dtype(preemph)
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr - c * prev
    fr = fr * povey_window(L).astype(dtype)[None, :]
    assert fr.dtype == dtype
    spec = scipy.fft.rfft(fr, n=n_fft, axis=1)
    assert spec.dtype == (np.complex64 if dtype == np.float32 else np.complex128), spec.dtype
    power = (spec.real * spec.real + spec.imag * spec.imag)[:, :n_fft // 2]
    assert power.dtype == dtype
    W = mel_weights(n_mels, n_fft, sample_rate, low_freq, high_freq).astype(dtype)
    E = power @ W.T
    assert E.dtype == dtype
    if not use_log:
        return E
    return np.log(np.maximum(E, dtype(FLT_EPSILON)))


def direct_dft_power(frame, n_fft):
    """O(N^2) float64 DFT of one (already windowed) frame, zero-padded to n_fft: |X[k]|^2 for k < n_fft / 2."""
    x = np.zeros(n_fft)
    x[:len(frame)] = frame
    k = np.arange(n_fft // 2)[:, None]
    n = np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * k * n / n_fft
    re, im = (x[None, :] * np.cos(ang)).sum(1), -(x[None, :] * np.sin(ang)).sum(1)
    return re * re + im * im


def cmvn_stats(x, dtype=np.float64):
    """x [T, n_mels] -> (mean, istd): biased variance about the mean, istd = 1 / sqrt(max(var, 1e-10))."""
    x = np.asarray(x).astype(dtype)
    mean = x.mean(axis=0, dtype=dtype)
    var = ((x - mean) ** 2).mean(axis=0, dtype=dtype)
    return mean, (dtype(1.0) / np.sqrt(np.maximum(var, dtype(1e-10)))).astype(dtype)


S1 = np.array([-2.0, -1.0, 0.0, 1.0, 2.0]) / 10.0
S2 = np.convolve(S1, S1)


def deltas(y, order, dtype=np.float64):
    """Kaldi add-deltas, window 2: y [T, n] -> [T, n (1 + order)]; each order filters the STATIC rows, index clamped."""
    y = np.asarray(y).astype(dtype)
    T = y.shape[0]
    blocks = [y]
    for k in range(1, order + 1):
        taps = (S1 if k == 1 else S2).astype(dtype)
        W = (len(taps) - 1) // 2
        acc = np.zeros_like(y)
        for d in range(-W, W + 1):
            acc = acc + taps[d + W] * y[np.clip(np.arange(T) + d, 0, T - 1)]
        blocks.append(acc)
    return np.concatenate(blocks, axis=1)


def finish(statics, t_max, order=0, cmvn="none", stats=None, masks=None, n_freq_masks=0, dtype=np.float64):
    """statics: list of [T_b, n_mels]; stats: (mean, istd) for "global"; masks: int [B, n_masks, 2] (start, width),
    frequency masks first -> [B, t_max, n_mels (1 + order)] in `dtype`."""
    n_mels = statics[0].shape[1]
    out = np.zeros((len(statics), t_max, n_mels * (1 + order)), dtype)
    for b, x in enumerate(statics):
        T = x.shape[0]
        if T == 0:
            continue
        y = np.asarray(x).astype(dtype)
        if cmvn == "utterance":
            mean, istd = cmvn_stats(y, dtype)
            y = (y - mean) * istd
        elif cmvn == "global":
            y = (y - np.asarray(stats[0]).astype(dtype)) * np.asarray(stats[1]).astype(dtype)
        f = deltas(y, order, dtype)
        if masks is not None:
            for m, (s0, w) in enumerate(np.asarray(masks[b])):
                if w <= 0:
                    continue
                if m < n_freq_masks:
                    for k in range(1 + order):
                        f[:, k * n_mels + max(s0, 0):k * n_mels + min(s0 + w, n_mels)] = 0
                else:
                    f[max(s0, 0):max(s0 + w, 0)] = 0
        out[b, :T] = f
    return out


def signals(seed=0, n=16000):
    """The inputs of the fbank tests (1 s at 16 kHz by default), int16-range float64: white noise; two sines plus noise; a
    sine on a DC offset plus unit noise; an amplitude ramp."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return {
        "white": rs.normal(0.0, 3000.0, n),
        "sines": 8000.0 * np.sin(2 * np.pi * 440.0 * t) + 3000.0 * np.sin(2 * np.pi * 3100.0 * t + 0.3) + rs.normal(0.0, 30.0, n),
        "dc": 6000.0 + 5000.0 * np.sin(2 * np.pi * 1000.0 * t) + rs.normal(0.0, 1.0, n),
        "ramp": np.linspace(10.0, 20000.0, n) * np.sin(2 * np.pi * 250.0 * t) + rs.normal(0.0, 5.0, n),
    }


def as_int16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def ratio(got, ref64_linear):
    """The tests' measure on linear mel energies: |got - ref| / the frame's largest mel energy -> [T, n_mels]."""
    fm = np.maximum(ref64_linear.max(axis=1, keepdims=True), np.finfo(np.float64).tiny)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64_linear) / fm


FRAME_TILE = 8          # ASR_FBANK_FRAME_TILE: the kernel's frames per workgroup


def fbank_cases():
    """The fbank inputs of tests/test_frontend_gpu.py - and of the allowance cap in tests/test_frontend_cpu.py, which runs
    over exactly this set: (name, [utterances], keyword arguments of fbank())."""
    sig = signals()
    k16 = dict(sample_rate=16000, L=400, S=160, n_fft=512, n_mels=80, low_freq=20.0, high_freq=8000.0)
    cases = [("signals_i16", [as_int16(v) for v in sig.values()], k16),
             ("signals_f32", [v.astype(np.float32) for v in sig.values()], k16)]
    rs = np.random.RandomState(7)
    counts = [400, 399, 559, 560, 561] + [400 + 160 * (t - 1) for t in (FRAME_TILE - 1, FRAME_TILE, FRAME_TILE + 1)]
    edges = [rs.normal(0.0, 2000.0, n) for n in counts]
    cases.append(("edges_i16", [as_int16(v) for v in edges], k16))            # (the utterance behind 399 starts odd)
    cases.append(("edges_f32", [v.astype(np.float32) for v in edges], k16))
    quarter = sig["sines"][:4000]
    for n_mels in (1, 23, 64, 65, 128):
        cases.append(("mels%d" % n_mels, [as_int16(quarter), as_int16(sig["white"][:2000])], dict(k16, n_mels=n_mels)))
    t8 = np.arange(4000) / 8000.0
    tel = 7000.0 * np.sin(2 * np.pi * 700.0 * t8) + rs.normal(0.0, 100.0, 4000)
    cases.append(("8k", [as_int16(tel), as_int16(tel[:1001])],
                  dict(sample_rate=8000, L=200, S=80, n_fft=256, n_mels=40, low_freq=20.0, high_freq=4000.0)))
    cases.append(("L_is_nfft", [as_int16(quarter)], dict(k16, L=512)))
    return cases

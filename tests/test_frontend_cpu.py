"""The front end without a GPU: the host arithmetic of hip_backend / frontend.py, the numpy restatement the GPU tests are
gated by (tests/frontend_ref.py) against independent forms, and the cap on the allowance that restatement may hand them."""
import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import frontend_ref as R


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    return hip_backend


@pytest.mark.parametrize("n", [0, 399, 400, 559, 560, 561, 16000])
def test_num_frames(hb, n):
    want = 1 + (n - 400) // 160 if n >= 400 else 0
    assert hb.fbank_num_frames(n, 400, 160) == want == R.num_frames(n) == hb.FbankPlan().num_frames(n)
    from frontend import Frontend
    assert Frontend({}).num_frames(n) == want


def test_plan_refuses_unsupported_shapes(hb):
    for kw in (dict(n_fft=1024), dict(n_fft=128, frame_length=100), dict(frame_length=513), dict(n_mels=129), dict(n_mels=0)):
        with pytest.raises(hb.UnsupportedShape):
            hb.FbankPlan(**kw)
    with pytest.raises(hb.UnsupportedShape):
        hb.fbank_plan_bytes(384)
    assert hb.fbank_plan_bytes(512) == 4 * (7 * 512 // 2 + 3 * 128)


def test_restatement_against_a_direct_dft():
    """One frame, float64: the restatement's rfft route against an O(N^2) DFT with the same window and weights."""
    x = R.signals()["sines"][:400]
    fr = x - x.mean()
    fr = (fr - 0.97 * np.concatenate([fr[:1], fr[:-1]])) * R.povey_window(400)
    want = R.mel_weights(80, 512, 16000, 20.0, 8000.0) @ R.direct_dft_power(fr, 512)
    got = R.fbank(x, np.float64, use_log=False)
    assert got.shape == (1, 80)
    assert np.abs(got[0] - want).max() <= 1e-11 * want.max()
    assert np.allclose(R.fbank(x, np.float64), np.log(np.maximum(want, R.FLT_EPSILON))[None], rtol=0, atol=1e-9)


@pytest.mark.parametrize("sr,n_fft,n_mels", [(16000, 512, 80), (16000, 512, 23), (8000, 256, 40), (16000, 512, 128)])
def test_mel_weights_sum_to_one_between_the_centres(sr, n_fft, n_mels):
    W = R.mel_weights(n_mels, n_fft, sr, 20.0, 0.5 * sr)
    pts = R.mel(20.0) + (R.mel(0.5 * sr) - R.mel(20.0)) * np.arange(n_mels + 2) / (n_mels + 1)
    m = R.mel(np.arange(n_fft // 2) * (sr / float(n_fft)))
    inside = (m >= pts[1]) & (m <= pts[-2])
    assert inside.sum() > n_fft // 4
    assert np.abs(W.sum(0)[inside] - 1.0).max() <= 1e-12
    assert (W >= 0).all() and (W.sum(0) <= 1.0 + 1e-12).all()


def test_product_tables_match_the_restatement(hb):
    """hip_backend.FbankPlan's packed [start, len] + weights table against the restatement's dense matrix, and its window."""
    for kw in (dict(), dict(sample_rate=8000, frame_length=200, frame_shift=80, n_fft=256, n_mels=40), dict(n_mels=128),
               dict(n_mels=1)):
        p = hb.FbankPlan(**kw)
        N = p.n_fft
        w = p.words
        assert np.array_equal(w[:p.frame_length].view(np.float32), R.povey_window(p.frame_length).astype(np.float32))
        assert not w[p.frame_length:N].any()
        o = 2 * N + N // 2
        start, ln, woff = w[o:o + 128], w[o + 128:o + 256], w[o + 256:o + 384]
        packed = w[o + 384:].view(np.float32)
        dense = np.zeros((p.n_mels, N // 2), np.float32)
        for j in range(p.n_mels):
            assert 0 <= start[j] and start[j] + ln[j] <= N // 2 and woff[j] + ln[j] <= N
            dense[j, start[j]:start[j] + ln[j]] = packed[woff[j]:woff[j] + ln[j]]
        want = R.mel_weights(p.n_mels, N, p.sample_rate, p.low_freq, p.high_freq).astype(np.float32)
        assert np.array_equal(dense, want)


def test_deltas_against_convolution():
    rs = np.random.RandomState(3)
    y = rs.normal(size=(40, 5))
    d = R.deltas(y, 2)
    assert d.shape == (40, 15) and np.array_equal(d[:, :5], y)
    for j in range(5):
        # np.convolve flips its kernel: correlate with the taps = convolve with the reversed taps
        c1 = np.convolve(y[:, j], R.S1[::-1], mode="valid")       # frames 2 .. T - 3
        c2 = np.convolve(y[:, j], R.S2[::-1], mode="valid")       # frames 4 .. T - 5
        assert np.allclose(d[2:-2, 5 + j], c1, rtol=0, atol=1e-14)
        assert np.allclose(d[4:-4, 10 + j], c2, rtol=0, atol=1e-14)
    assert np.allclose(R.S2 * 100, [4, 4, 1, -4, -10, -4, 1, 4, 4])
    one = R.deltas(y[:1], 2)                                       # a single frame: every clamped tap reads it, taps sum to 0
    assert np.abs(one[:, 5:]).max() <= 1e-15


def test_draw_masks():
    from frontend import Frontend
    fe = Frontend(dict(specaug=dict(n_freq_masks=2, max_freq_width=27, n_time_masks=2, max_time_width=40)))
    assert fe.n_masks == 4 and fe.output_dim == 80
    lens = [98, 61, 40, 7, 1, 0]
    one = [fe.draw_masks(11, 3, i, t) for i, t in enumerate(lens)]
    again = [fe.draw_masks(11, 3, i, t) for i, t in enumerate(lens)]
    for a, b, t in zip(one, again, lens):
        assert a.dtype == np.int32 and a.shape == (4, 2) and np.array_equal(a, b)
        assert (a[:, 1] >= 0).all() and (a[:, 0] >= 0).all()
        assert (a[:2, 1] <= 27).all() and (a[:2].sum(1) <= 80).all()
        assert (a[2:, 1] <= min(40, t)).all() and (a[2:].sum(1) <= max(t, 0)).all()
    others = [fe.draw_masks(11, 4, 0, 98), fe.draw_masks(12, 3, 0, 98), fe.draw_masks(11, 3, 1, 98)]
    assert any(not np.array_equal(one[0], o) for o in others)          # (the seed, the batch and the row all enter)
    # two ranks draw their strided rows; together: the one-process draw
    import parallel
    union = {}
    for rank in range(2):
        for i in parallel.shard_indices(len(lens), rank, 2):
            union[i] = fe.draw_masks(11, 3, i, lens[i])
    assert sorted(union) == list(range(len(lens)))
    assert all(np.array_equal(union[i], one[i]) for i in union)
    assert Frontend({}).n_masks == 0 and Frontend(dict(delta_order=2)).output_dim == 240


def test_feed_with_a_front_end_refuses_the_cpu():
    from feed import DeviceFeed
    from frontend import Frontend
    items = [[(np.zeros(1600, np.int16), [3, 4])]]
    with pytest.raises(RuntimeError):
        DeviceFeed(items, "cpu", frontend=Frontend({}), thread=False)
    with pytest.raises(RuntimeError):
        Frontend({})(torch.zeros(1600, dtype=torch.int16), [0, 1600])


def test_dataset_filters_by_frames_not_samples():
    from dataset import DictDataset, synthetic_waveforms
    from frontend import Frontend
    fe = Frontend({})
    data = synthetic_waveforms(6, 30, 0.5, seed=2)
    assert all(v["feature"].dtype == np.int16 and v["feature"].ndim == 1 for v in data.values())
    cfg = dict(min_feature_length=1, max_feature_length=40, min_text_length=1, max_text_length=100)
    assert len(DictDataset(data, cfg)) == 0                              # sample counts are all above 40
    ds = DictDataset(data, cfg, frames_of=fe.frames_of)
    frames = [fe.num_frames(f.shape[0]) for f, _ in ds]
    assert len(ds) == sum(1 <= fe.num_frames(v["feature"].shape[0]) <= 40 for v in data.values()) > 0
    assert frames == sorted(frames)


def test_solver_checks_input_dim_against_the_front_end():
    import solver
    with pytest.raises(ValueError, match="input_dim"):
        solver.Solver(dict(logdir="/nonexistent", input_dim=80, frontend=dict(delta_order=2)))


def test_allowance_cap():
    """The GPU gate is a multiple of the float32 restatement's own error, so that error is capped here, over the exact
    inputs of the GPU test: |E32 - E64| / the frame's largest mel energy <= 5e-7 (linear energies)."""
    worst = {}
    for name, utts, kw in R.fbank_cases():
        w = 0.0
        for u in utts:
            ref = R.fbank(u, np.float64, use_log=False, **kw)
            if ref.shape[0]:
                w = max(w, float(R.ratio(R.fbank(u, np.float32, use_log=False, **kw), ref).max()))
        worst[name] = w
    print({k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) <= 5e-7, worst

"""Speed perturbation on the GPU (csrc/resample.hip) against the float64 restatement of tests/resample_ref.py.

Parity is per element: |got - ref64| <= (taps + 2) * 2^-24 * sum_k |h[j][k]| |x[..]| and nothing more - one unit for the
taps' rounding to fp32, one per step of the running sum, one to spare; tests/test_resample_cpu.py holds the float32
restatement to the same allowance over the same inputs.  Every case prints its worst error / allowance as a
`resample-parity` line (profiles/resample_parity.txt is that output)."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import resample_ref as R

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 700


@pytest.fixture(scope="module")
def hb():
    entry.build()
    import hip_backend
    assert torch.cuda.is_available()
    return hip_backend


@pytest.fixture(scope="module")
def plan(hb):
    return hb.ResamplePlan(R.SAMPLE_RATE, R.FACTORS)


_CASES = {}
_REF = {}


def _cases(hb):
    if not _CASES:
        _CASES.update({name: (utts, fidx) for name, utts, fidx in R.cases(hb.RESAMPLE_TILE)})
    return _CASES


def _refs(hb, name):
    """float64 outputs, magnitudes and tap counts of every row of a case, computed once (float32 inputs hold the same values)."""
    if name not in _REF:
        utts, fidx = _cases(hb)[name]
        _REF[name] = [R.resample(x, *R.ratio(R.FACTORS[f])) for x, f in zip(utts, fidx)]
    return _REF[name]


def _launch(hb, plan, utts, fidx, in_tail=None, gap=0, device_index=True):
    """One launch -> (rows: list of numpy outputs, the whole output buffer as numpy, out offsets).  The packed input is
    followed INSIDE the tensor handed over by TAIL elements of `in_tail` (None: no tail), the output by TAIL canaries, and
    `gap` canaries lie between the rows of the output."""
    dtype = utts[0].dtype
    total = sum(len(u) for u in utts)
    buf = np.zeros(total + (TAIL if in_tail is not None else 0), dtype)
    offs = [0]
    for u in utts:
        buf[offs[-1]:offs[-1] + len(u)] = u
        offs.append(offs[-1] + len(u))
    if in_tail is not None:
        buf[total:] = in_tail
    n_out = [plan.out_samples(len(u), f) for u, f in zip(utts, fidx)]
    out_offs = [0]
    for n in n_out:
        out_offs.append(out_offs[-1] + n + gap)
    out = torch.full((out_offs[-1] + TAIL,), CANARY, device="cuda")
    fi = torch.tensor(fidx, dtype=torch.int32).cuda() if device_index else list(fidx)
    hb.resample(plan, torch.from_numpy(buf).cuda(), torch.tensor(offs, dtype=torch.int64).cuda(), fi,
                torch.tensor(out_offs, dtype=torch.int64).cuda(), out, max_out=max(n_out))
    whole = out.cpu().numpy()
    return [whole[o:o + n] for o, n in zip(out_offs, n_out)], whole, out_offs


CASE_NAMES = ["mixed", "tile_edges", "full_scale_noise", "neighbours", "batch_of_one"]


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_parity_per_element(hb, plan, name, dtype):
    utts, fidx = _cases(hb)[name]
    rows, whole, out_offs = _launch(hb, plan, [u.astype(dtype) for u in utts], fidx)
    worst = 0.0
    for b, (got, (ref, mag, taps)) in enumerate(zip(rows, _refs(hb, name))):
        assert got.shape == ref.shape == (R.out_samples(len(utts[b]), *R.ratio(R.FACTORS[fidx[b]])),)
        err, tol = np.abs(got.astype(np.float64) - ref), R.allowance(mag, taps)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("resample-parity %-17s %-7s rows %2d  worst error / allowance %.3f" % (name, np.dtype(dtype).name, len(rows), worst))
    assert worst <= 1.0, (name, worst)
    assert (whole[out_offs[-1]:] == CANARY).all()


def test_tile_edge_lengths(hb, plan):
    utts, _ = _cases(hb)["tile_edges"]
    T = hb.RESAMPLE_TILE
    assert [plan.out_samples(len(u), 0) for u in utts] == [T - 1, T, 2 * T + 1]


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_factor_one_rows_are_copied_by_value(hb, plan, dtype):
    rs = np.random.RandomState(3)
    if dtype == np.int16:
        a = rs.randint(-32768, 32768, 2500).astype(np.int16)
        a[:2] = (-32768, 32767)
    else:
        a = (rs.randn(2500) * 1000).astype(np.float32)
        a[:3] = (-0.0, 1e-40, 3.4e38)                       # a signed zero, a subnormal, a value near the largest
    b = a[:1100][::-1].copy()
    other = (rs.randn(1500) * 3000).astype(dtype)
    rows, _, _ = _launch(hb, plan, [other, a, other[:7].copy(), b], [0, 1, 2, 1])
    view = np.int32
    assert np.array_equal(rows[1].view(view), a.astype(np.float32).view(view))
    assert np.array_equal(rows[3].view(view), b.astype(np.float32).view(view))
    assert len(rows[0]) == plan.out_samples(1500, 0) and np.abs(rows[0]).max() > 0


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_bounds(hb, plan, dtype):
    """Nothing behind in_offsets[B] is read, nothing behind out_offsets[B] or between the rows is written: a loud tail inside
    the input tensor changes no output, the canaries stay."""
    utts, fidx = _cases(hb)["mixed"]
    utts = [u.astype(dtype) for u in utts]
    plain, _, _ = _launch(hb, plan, utts, fidx)
    rows, whole, out_offs = _launch(hb, plan, utts, fidx, in_tail=32767 if dtype == np.int16 else np.nan, gap=3)
    mask = np.ones(whole.size, bool)
    for b, r in enumerate(rows):
        assert np.array_equal(r.view(np.int32), plain[b].view(np.int32)), b
        mask[out_offs[b]:out_offs[b] + len(r)] = False
    assert mask.sum() == TAIL + 3 * len(rows) and (whole[mask] == CANARY).all()


def test_two_runs_give_the_same_bits(hb, plan):
    utts, fidx = _cases(hb)["mixed"]
    first, _, _ = _launch(hb, plan, utts, fidx)
    again, _, _ = _launch(hb, plan, utts, fidx)
    with hb.deterministic():
        det, _, _ = _launch(hb, plan, utts, fidx)
    host, _, _ = _launch(hb, plan, utts, fidx, device_index=False)
    for a, b, c, d in zip(first, again, det, host):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32))
        assert np.array_equal(a.view(np.int32), d.view(np.int32))


def test_refused_shapes_launch_nothing(hb, plan):
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    offs = torch.tensor([0, 30, 64], dtype=torch.int64).cuda()
    out = torch.full((256,), CANARY, device="cuda")
    before = hb.LAUNCHES["resample"]
    for bad in ([0, len(plan)], [-1, 0], [0]):
        with pytest.raises(hb.UnsupportedShape):
            hb.resample(plan, x, offs, bad, offs, out)
    B = 65536
    many = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(hb.UnsupportedShape):
        hb.resample(plan, x, many, torch.zeros(B, dtype=torch.int32, device="cuda"), many, out)
    with pytest.raises(RuntimeError):
        hb.resample(plan, x.cpu(), offs, [0, 0], offs, out)
    # the C entry itself: a plan beyond the limits, a dtype code that is neither of the two
    lib, c_p = hb.load(), ctypes.c_void_p
    fi = torch.zeros(2, dtype=torch.int32, device="cuda")
    tables = plan.on("cuda")

    def call(geometry, dtype_code):
        g = np.ascontiguousarray(geometry, dtype=np.int32)
        return lib.asr_resample_f32(2, 64, c_p(x.data_ptr()), dtype_code, 64, c_p(offs.data_ptr()), c_p(fi.data_ptr()),
                                    c_p(offs.data_ptr()), g.shape[0], c_p(g.ctypes.data), c_p(tables.data_ptr()),
                                    tables.numel() * 4, c_p(out.data_ptr()), out.numel(), hb.stream())
    wide = plan.geometry.copy()
    wide[0, 1] = hb.RESAMPLE_MAX_PHASES + 1
    assert call(wide, hb.SAMPLES_I16) == hb.ASR_E_SHAPE
    assert call(np.tile(plan.geometry[:1], (hb.RESAMPLE_MAX_FACTORS + 1, 1)), hb.SAMPLES_I16) == hb.ASR_E_SHAPE
    assert call(plan.geometry, 2) == hb.ASR_E_SHAPE and call(plan.geometry, -1) == hb.ASR_E_SHAPE
    torch.cuda.synchronize()
    assert hb.LAUNCHES["resample"] == before and (out == CANARY).all()


# ------------------------------------------------------------------------------------------------ Frontend and the feed
def _items(n=6, seed=3, dtype=np.int16):
    from dataset import synthetic_waveforms
    data = synthetic_waveforms(n, 9, 0.3, seed=seed, dtype=dtype)
    return [(v["feature"], v["token_ids"]) for v in data.values()]


FE_CFG = dict(n_mels=8, delta_order=0, cmvn="utterance",
              specaug=dict(n_freq_masks=1, max_freq_width=3, n_time_masks=1, max_time_width=6))
SPEEDS = [0.9, 1.0, 1.1]


def _pack(items):
    offs = np.concatenate([[0], np.cumsum([len(f) for f, _ in items])])
    return torch.from_numpy(np.concatenate([f for f, _ in items])).cuda(), offs.tolist()


def _direct(fe, items, masks=None):
    """Today's batch: sorted by raw sample count, no perturbation."""
    items = sorted(items, key=lambda it: -len(it[0]))
    samples, offs = _pack(items)
    return fe(samples, offs, masks=masks)


def _direct_speed(fe, items, speed_seed, mask_seed, batch_index):
    """The perturbed batch computed directly: draw by collated row, sort by perturbed count, Frontend.__call__."""
    draws = [fe.draw_speed(speed_seed, batch_index, i) for i in range(len(items))]
    pert = [fe.perturbed_samples(len(f), d) for (f, _), d in zip(items, draws)]
    order = sorted(range(len(items)), key=lambda i: -pert[i])
    items, fidx, pert = [items[i] for i in order], [draws[i] for i in order], [pert[i] for i in order]
    frames = [fe.num_frames(p) for p in pert]
    masks = None
    if mask_seed is not None:
        masks = np.stack([fe.draw_masks(mask_seed, batch_index, r, T) for r, T in enumerate(frames)])
    samples, offs = _pack(items)
    xs, ilens = fe(samples, offs, masks=masks, factor_index=fidx)
    return xs, ilens, items, fidx, frames, masks


def test_frontend_run_with_factor_indices(hb):
    """The composition adds nothing of its own: Frontend with factor indices equals, bit for bit, Frontend on the GPU-resampled
    samples handed in as a float32 waveform batch; four launches; frame counts from the perturbed sample counts."""
    from frontend import Frontend
    fe = Frontend(dict(FE_CFG, specaug=None, delta_order=1, speed_perturb=SPEEDS))
    items = _items(5, seed=8)
    fidx = [0, 2, 1, 0, 2]
    samples, offs = _pack(items)
    before = dict(hb.LAUNCHES)
    xs, ilens = fe(samples, offs, factor_index=fidx)
    delta = {k: hb.LAUNCHES[k] - before.get(k, 0) for k in ("resample", "fbank", "feat_cmvn_stats", "feat_finish")}
    assert delta == dict(resample=1, fbank=1, feat_cmvn_stats=1, feat_finish=1)
    counts = [-(-new * len(f) // orig) for (f, _), (orig, new) in zip(items, (R.ratio(SPEEDS[i]) for i in fidx))]
    assert ilens == [fe.num_frames(c) for c in counts] and xs.shape == (5, max(ilens), 16)
    out_offs = np.concatenate([[0], np.cumsum(counts)])
    resampled = torch.empty(int(out_offs[-1]), device="cuda")
    hb.resample(fe.resample_plan, samples, torch.tensor(offs, dtype=torch.int64).cuda(), fidx,
                torch.tensor(out_offs, dtype=torch.int64).cuda(), resampled, max_out=max(counts))
    want, want_lens = fe(resampled, out_offs.tolist())
    assert want_lens == ilens and torch.equal(xs, want)
    plain, plain_lens = fe(samples, offs)
    assert plain_lens != ilens
    with pytest.raises(hb.UnsupportedShape):
        fe(samples, offs, factor_index=[0, 1, 2, 3, 0])
    with pytest.raises(ValueError):
        Frontend(FE_CFG)(samples, offs, factor_index=fidx)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("thread", [False, True])
def test_training_feed_perturbs(hb, dtype, thread):
    from feed import DeviceFeed
    from frontend import Frontend
    fe = Frontend(dict(FE_CFG, speed_perturb=SPEEDS))
    batches = [_items(6, seed=3, dtype=dtype), _items(7, seed=4, dtype=dtype)]

    def feeds(**kw):
        np.random.seed(21)                                   # the feeds take their mask and speed seeds from this stream
        return DeviceFeed(batches, "cuda", frontend=fe, thread=thread, train=True, **kw)
    whole = feeds()
    assert whole.speed_seed is not None and whole.mask_seed is not None
    shards = [iter(feeds(rank=rank, world=2)) for rank in range(2)]
    seen, n = set(), 0
    for bi, (items, (xs, ilens, ys)) in enumerate(zip(batches, whole)):
        want, want_lens, order, fidx, frames, masks = _direct_speed(fe, items, whole.speed_seed, whole.mask_seed, bi)
        torch.cuda.synchronize()
        assert ilens == want_lens == frames == sorted(ilens, reverse=True)
        assert torch.equal(xs, want) and xs.shape[1] == max(frames)
        assert [y.tolist() for y in ys] == [t for _, t in order]
        assert (masks[:, 1, 0] + masks[:, 1, 1] <= np.asarray(frames)).all() and masks[:, :, 1].max() > 0
        assert ilens != [fe.num_frames(len(f)) for f, _ in order]
        seen.update(fidx)
        for rank in range(2):
            shard, il, ys_r = next(shards[rank])
            torch.cuda.synchronize()
            assert il == ilens[rank::2] and shard.info["t_max"] == xs.shape[1] and shard.info["b_global"] == len(items)
            assert torch.equal(shard.xs, xs[rank::2])
            assert [y.tolist() for y in ys_r] == [y.tolist() for y in ys[rank::2]]
        n += 1
    assert n == 2 and len(seen) > 1
    for it in shards:
        assert next(it, None) is None


def test_other_feeds_give_todays_batch(hb):
    """train=False with `speed_perturb`, and a training feed whose front end has no such key: today's batch, bit for bit,
    today's draws from the process's numpy stream, and no resample launch."""
    from feed import DeviceFeed
    from frontend import Frontend
    fe, plain = Frontend(dict(FE_CFG, speed_perturb=SPEEDS)), Frontend(FE_CFG)
    items = _items(7, seed=6)
    before = hb.LAUNCHES["resample"]
    np.random.seed(21)
    first, second = int(np.random.randint(0, 2 ** 31 - 1)), int(np.random.randint(0, 2 ** 31 - 1))
    np.random.seed(21)
    feed = DeviceFeed([items], "cuda", frontend=plain, thread=False, train=True)
    assert feed.mask_seed == first and feed.speed_seed is None
    assert int(np.random.randint(0, 2 ** 31 - 1)) == second           # one draw taken, as before
    xs, ilens, _ = next(iter(feed))
    order = sorted(items, key=lambda it: -len(it[0]))
    masks = np.stack([plain.draw_masks(first, 0, i, plain.num_frames(len(f))) for i, (f, _) in enumerate(order)])
    want, want_lens = _direct(plain, items, masks=masks)
    assert ilens == want_lens and torch.equal(xs, want)
    np.random.seed(21)
    speedy = DeviceFeed([items], "cuda", frontend=fe, thread=False, train=True)
    assert (speedy.mask_seed, speedy.speed_seed) == (first, second)   # the speed seed comes after the mask seed
    clean, clean_lens = _direct(plain, items)
    for kw in (dict(), dict(kind="speech")):
        np.random.seed(21)
        feed = DeviceFeed([items], "cuda", frontend=fe, thread=False, train=False, **kw)
        assert feed.mask_seed is None and feed.speed_seed is None
        assert int(np.random.randint(0, 2 ** 31 - 1)) == first        # nothing taken
        batch = next(iter(feed))
        assert batch.ilens == clean_lens and torch.equal(batch.xs, clean)
    assert hb.LAUNCHES["resample"] == before


def test_e2e_forward_backward_on_a_perturbed_batch(hb):
    import synth
    import model as M
    from feed import DeviceFeed
    from frontend import Frontend
    cfg = dict(synth.TINY)
    fe = Frontend(dict(FE_CFG, speed_perturb=SPEEDS))
    assert fe.output_dim == cfg["input_dim"]
    net = M.E2E(labeldist=synth.labeldist(cfg["output_dim"], 12), **cfg).to("cuda")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.e2e_weights(cfg, 11).items()})
    net.train()
    np.random.seed(5)
    before = hb.LAUNCHES["resample"]
    xs, ilens, ys = next(iter(DeviceFeed([_items(3, seed=2)], "cuda", frontend=fe, thread=False, train=True)))
    assert hb.LAUNCHES["resample"] == before + 1
    _, lp, _, _ = net(xs, ilens, ys)
    loss = -lp.mean()
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(xs).all()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)

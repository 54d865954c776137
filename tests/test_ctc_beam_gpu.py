"""The CTC prefix beam search kernel on the GPU (csrc/ctc_beam.hip, hb.ctc_beam, ops.ctc_beam) against the
dictionary-based restatement (tests/ctc_beam_ref.py) over the grid V x K x T' x logit scale, B = 3 ragged with an utterance of
no frames, ld = V + 3, NaN behind every utterance and in the padding columns - and over the shapes on either side of the
kernel's switches (one wave / four, staged tokens / tokens read from memory, history in LDS / in the workspace).

Per utterance: (1) the hypotheses are well-formed and distinct; (2) score[k] <= -asr_ctc_loss_fwd(hyp[k]) + allowance - the
beam's mass of a labelling is a subset of its paths; (3) where the restatement is decisive the hypotheses, their order and -
within the allowance - their scores are the float64 restatement's.  The allowance is the restatement's (ctc_beam_ref.judge):
4 x the float32 restatement's error against float64, at least 8 fp32 ulps of the score.  Undecided utterances (at most 10 %
of the grid: tests/test_ctc_beam_cpu.py holds the seeds to that without a GPU) are left out of (3) only."""
import numpy as np
import pytest
import torch

import ctc_beam_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _search(z, lens, V, K):
    """z float32 [B, T, V + 3] numpy (ld = V + 3), lens -> (hyp, hyp_len, score) on the host, and the device logits view."""
    import hip_backend as hb
    import ops
    zd = torch.from_numpy(z).cuda()
    view = zd[:, :, :V]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    hyp, hyp_len, score = ops.ctc_beam(view, lens_dev, K)
    torch.cuda.synchronize()
    return hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy(), view, lens_dev


def _loss_bound(view, lens, hyps):
    """-asr_ctc_loss_fwd of every non-empty hypothesis (b, labels) in one call; the empty labelling's log-likelihood is the
    blank path's, summed on the host in float64."""
    import ops
    out = {}
    rows = [(b, h) for b, h in hyps if len(h) > 0]
    if rows:
        idx = torch.tensor([b for b, _ in rows], device="cuda")
        zz = view[idx].contiguous()
        lens_dev = torch.tensor([int(lens[b]) for b, _ in rows], dtype=torch.int32, device="cuda")
        labels = torch.tensor([c for _, h in rows for c in h], dtype=torch.long, device="cuda")
        nll = ops.ctc_loss(zz, lens_dev, labels, [len(h) for _, h in rows], zero_infinity=False).cpu().numpy()
        for (b, h), v in zip(rows, nll):
            out[(b, h)] = -float(v)
    host = view.cpu().numpy().astype(np.float64)
    for b, h in hyps:
        if len(h) == 0:
            out[(b, h)] = float(R.log_probs(host[b, :lens[b]])[:, 0].sum()) if lens[b] > 0 else 0.0
    return out


def _check_case(V, K, T, scale, worst):
    z, lens = R.grid_case(V, K, T, scale)
    hyp, hyp_len, score, view, _ = _search(z, lens, V, K)
    verdict = R.judge(V, K, T, scale)
    got = []
    for b in range(3):
        rows = []
        for k in range(K):
            n = int(hyp_len[b, k])
            if n < 0:                                            # an unused slot: behind every used one, -inf, all padding
                assert np.isneginf(score[b, k]) and (hyp[b, k] == -1).all() and (hyp_len[b, k:] == -1).all()
                continue
            h = tuple(int(c) for c in hyp[b, k, :n])
            assert n <= lens[b] and all(1 <= c < V for c in h) and (hyp[b, k, n:] == -1).all(), (b, k, h)
            assert np.isfinite(score[b, k])
            rows.append((h, float(score[b, k])))
        assert len({h for h, _ in rows}) == len(rows) >= 1, "a hypothesis twice, or none"
        assert all(a[1] >= c[1] for a, c in zip(rows, rows[1:])), "scores not descending"
        got.append(rows)
    assert got[2] == [((), 0.0)]                                 # no frames: the empty hypothesis at score 0
    bound = _loss_bound(view, lens, [(b, h) for b in range(3) for h, _ in got[b]])
    for b in range(3):
        allow = verdict[b]["allowance"]
        for h, s in got[b]:
            assert s <= bound[(b, h)] + allow, "utterance %d %r: score %.9g above the labelling's %.9g + %.3g" % (
                b, h, s, bound[(b, h)], allow)
        if not verdict[b]["decisive"]:
            continue
        ref = verdict[b]["ref"]
        assert [h for h, _ in got[b]] == ref["hyps"], (V, K, T, scale, b)
        err = max(abs(s - float(r)) for (_, s), r in zip(got[b], ref["scores"]))
        worst[0] = max(worst[0], err / allow if allow > 0 else (0.0 if err == 0 else np.inf))
        assert err <= allow, "utterance %d: score error %.3g above %.3g" % (b, err, allow)


@pytest.mark.parametrize("V", R.GRID_V)
@pytest.mark.parametrize("K", R.GRID_K)
def test_grid_against_the_restatement(hb, V, K):
    worst = [0.0]
    for T in R.GRID_T:
        for scale in R.GRID_SCALE:
            _check_case(V, K, T, scale, worst)
    print("V %d K %d: worst score error / allowance %.3f" % (V, K, worst[0]))


@pytest.mark.parametrize("case", R.EXTRA, ids=lambda c: "V%d-K%d-T%d-x%g" % c)
def test_either_side_of_the_switches(hb, case):
    worst = [0.0]
    _check_case(*case, worst)
    print("%r: worst score error / allowance %.3f" % (case, worst[0]))


@pytest.mark.parametrize("K", [1, 2, 4, 16])
def test_tie_rule_on_the_device(hb, K):
    """T' = 1 on all-equal logits: every candidate ties exactly; the empty prefix, then the tokens 1 .. K - 1, all at the
    same bits."""
    V = 20
    z = np.zeros((2, 1, V + 3), dtype=np.float32)
    z[:, :, V:] = np.nan
    hyp, hyp_len, score, _, _ = _search(z, [1, 1], V, K)
    for b in range(2):
        assert hyp_len[b].tolist() == [0] + [1] * (K - 1)
        assert hyp[b, :, 0].tolist() == [-1] + list(range(1, K))
        assert (score[b] == score[b, 0]).all()
        assert abs(float(score[b, 0]) + np.log(V)) <= 8 * np.spacing(np.float32(np.log(V)))


def test_merge_case_on_the_device(hb):
    """tests/test_ctc_beam_cpu.py::test_merge_case on the kernel: () . 1 re-enters a beam that holds (1)."""
    z = np.full((1, 2, 2 + 3), np.nan, dtype=np.float32)
    z[0, :, :2] = np.log(np.array([[0.6, 0.4], [0.3, 0.7]]))
    hyp, hyp_len, score, _, _ = _search(z, [2], 2, 4)
    assert hyp_len[0].tolist() == [1, 0, -1, -1] and hyp[0, 0].tolist() == [1, -1] and (hyp[0, 1:] == -1).all()
    want = np.log(np.array([0.82, 0.18]))
    assert np.abs(score[0, :2] - want).max() <= 8 * np.spacing(np.float32(np.abs(want).max()))
    assert np.isneginf(score[0, 2:]).all()
    z3 = np.full((1, 3, 3 + 3), np.nan, dtype=np.float32)
    z3[0, :, :3] = np.log(np.array([[0.5, 0.4, 0.1], [0.2, 0.1, 0.7], [0.3, 0.1, 0.6]]))
    hyp, hyp_len, score, _, _ = _search(z3, [3], 3, 16)
    mass = R.enumerate_paths(z3[0, :, :3].astype(np.float64))
    got = {tuple(int(c) for c in hyp[0, k, :hyp_len[0, k]]): float(score[0, k]) for k in range(16) if hyp_len[0, k] >= 0}
    assert set(got) == set(mass)
    for h, s in got.items():
        assert abs(s - mass[h]) <= 16 * np.spacing(np.float32(abs(mass[h]))), (h, s, mass[h])


def test_two_runs_give_the_same_bits_and_two_launches(hb):
    import ops
    z, lens = R.grid_case(34, 4, 100, 1.0)
    zd = torch.from_numpy(z).cuda()[:, :, :34]
    lens_dev = hb.to_device_i32([int(n) for n in lens], "cuda")
    hb.LAUNCHES.clear()
    a = ops.ctc_beam(zd, lens_dev, 4)
    assert hb.LAUNCHES["ctc_beam"] == 1 and hb.LAUNCHES["ctc_beam_launch"] == 2
    with hb.deterministic(True):
        b = ops.ctc_beam(zd, lens_dev, 4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.int32 and a[2].dtype == torch.float32 and a[0].is_cuda


def test_argument_errors(hb):
    import ops
    z = torch.zeros(2, 5, 6, device="cuda")
    lens = hb.to_device_i32([5, 3], "cuda")
    for K in (0, hb.BEAM_KMAX + 1):
        with pytest.raises(hb.UnsupportedShape):
            ops.ctc_beam(z, lens, K)
    with pytest.raises(hb.UnsupportedShape):
        ops.ctc_beam(z[:, :, :1], lens, 2)
    rc = hb.load().asr_ctc_beam_f32(2, 5, 1, 2, hb.ptr(z), 6, hb.ptr(lens), hb.ptr(z), hb.ptr(z), hb.ptr(z), hb.ptr(z), hb.stream())
    assert rc == -2

"""The star CTC loss without a GPU: the torch restatement (tests/ctc_star_ref.py) is checked three ways - against a brute-force
enumeration of every state sequence, against torch.nn.functional.ctc_loss where the stars are closed or priced out, and
against the inequality nll_star <= nll_ctc - then the case the loss exists for, and the C ABI's declarations."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_star_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _ctc(z, lens, labels, zero_infinity=False):
    ys = torch.tensor([v for y in labels for v in y], dtype=torch.long)
    return F.ctc_loss(F.log_softmax(z, -1).transpose(0, 1), ys, torch.tensor(lens), torch.tensor([len(y) for y in labels]),
                      blank=0, reduction="none", zero_infinity=zero_infinity)


def _brute(z, labels, penalty):
    """-log of the sum, over ALL sequences of T states, of exp(summed emissions) for those the definition admits - the
    predecessor rule is read per step, nothing is shared with the recursion but the rule itself."""
    T, V = z.shape
    x = z - torch.logsumexp(z, -1, keepdim=True)
    nb = torch.logsumexp(z[:, 1:], -1) - torch.logsumexp(z, -1)
    st = R.states(labels)

    def emission(t, s):
        kind, g = s
        if kind == R.BLANK:
            return float(x[t, 0])
        if kind == R.LABEL:
            return float(x[t, labels[g - 1]])
        return float(nb[t]) + penalty

    total = 0.0
    for path in itertools.product(st, repeat=T):
        if path[0] not in R.initial(labels) or path[-1] not in R.final(labels):
            continue
        if any(path[t - 1] not in R.predecessors(labels, *path[t]) for t in range(1, T)):
            continue
        score = sum(emission(t, s) for t, s in enumerate(path))
        if score > -INF:
            total += math.exp(score)
    return -math.log(total) if total > 0 else INF


def test_reference_equals_brute_force_enumeration():
    """T <= 4, V = 3, L <= 2, every label sequence (equal neighbours included), penalties 0, -0.7 and -inf: S^T <= 8^4
    sequences per case.  float64 on both sides: 1e-12 relative."""
    rs = np.random.RandomState(3)
    n = 0
    for T in (1, 2, 3, 4):
        for labels in ([], [1], [2], [1, 2], [2, 2], [1, 1]):
            z = torch.from_numpy(rs.normal(0, 2, size=(T, 3)))
            for pen in (0.0, -0.7, -INF):
                want = _brute(z, labels, pen)
                got, feasible = R.star_ctc_nll(z.unsqueeze(0), [T], [labels], [pen], zero_infinity=False)
                assert bool(feasible[0]) == (T >= R.needs_frames(labels)), (T, labels)
                if want == INF:
                    assert float(got[0]) == INF, (T, labels, pen)
                else:
                    assert abs(float(got[0]) - want) <= 1e-12 * max(1.0, abs(want)), (T, labels, pen, float(got[0]), want)
                n += 1
    assert n == 72


def _batch(seed, V=6):
    rs = np.random.RandomState(seed)
    utts = [(1, []), (1, [1]), (9, []), (3, [2, 2]), (2, [1, 3]), (5, [2, 2, 2, 4]), (12, [3] * 5), (14, [1, 2, 3, 3, 4, 5]),
            (30, [int(v) for v in rs.randint(1, V, size=11)])]
    T = max(t for t, _ in utts)
    z = torch.from_numpy(rs.normal(0, 3, size=(len(utts), T, V)))
    return z, [t for t, _ in utts], [y for _, y in utts]


@pytest.mark.parametrize("penalty", [-80.0, -INF])
def test_closed_stars_are_the_ctc_loss(penalty):
    """penalty = -inf closes the star states; at -80 a frame in a star costs e^-80 against a frame on a token of probability
    >= e^-20 here: both equal F.ctc_loss in float64 to 1e-12 relative, value and gradient; the infeasible row is +inf in
    both, and 0 with a zero gradient under zero_infinity."""
    z, lens, labels = _batch(5)
    zs, zc = z.clone().requires_grad_(), z.clone().requires_grad_()
    want = _ctc(zc, lens, labels)
    got, feasible = R.star_ctc_nll(zs, lens, labels, [penalty] * len(lens), zero_infinity=False)
    assert feasible.tolist() == torch.isfinite(want).tolist() and int((~feasible).sum()) == 1
    assert bool(torch.isinf(got[~feasible]).all())
    g, w = got[feasible].detach(), want[feasible].detach()
    assert float(((g - w).abs() / w.abs().clamp(min=1.0)).max()) <= 1e-12
    got0, _ = R.star_ctc_nll(zs, lens, labels, [penalty] * len(lens), zero_infinity=True)
    assert float(got0.detach()[~feasible].abs().max()) == 0.0
    got0.sum().backward()
    _ctc(zc, lens, labels, zero_infinity=True).sum().backward()
    assert bool(torch.isfinite(zs.grad).all())
    assert float((zs.grad - zc.grad).abs().max()) <= 1e-12 * float(zc.grad.abs().max())
    bad = int((~feasible).nonzero()[0])
    assert not bool(zs.grad[bad].any())
    for i, t in enumerate(lens):
        assert not bool(zs.grad[i, t:].any())


def test_star_never_costs_more_than_ctc():
    """Every CTC path is a star path with the same emissions: nll_star <= nll_ctc on every feasible row, at every penalty;
    and a lower penalty never lowers the loss.  float32 too (the yardstick's dtype), with its rounding: 1e-5 relative."""
    z, lens, labels = _batch(6)
    want = _ctc(z, lens, labels)
    last = None
    for pen in (0.0, -0.25, -1.0, -5.0):
        got, feasible = R.star_ctc_nll(z, lens, labels, [pen] * len(lens), zero_infinity=False)
        assert bool((got[feasible] <= want[feasible] + 1e-12).all()), pen
        if last is not None:
            assert bool((got[feasible] >= last[feasible] - 1e-12).all()), pen
        last = got
        got32, _ = R.star_ctc_nll(z.float(), lens, labels, [pen] * len(lens), zero_infinity=False)
        assert got32.dtype == torch.float32
        assert float(((got32.double() - got)[feasible].abs() / got[feasible].abs().clamp(min=1.0)).max()) <= 1e-5


def test_partial_transcript_of_a_peaked_posterior():
    """8 labels over 24 frames, each label one frame and two blank frames, the frame's token 10 nats above every other; the
    transcript lacks labels 4 .. 6.  Plain CTC must put three label frames on the blank, 10 nats each: 30.  The star lattice
    spends them in a star at the penalty, 0.5 each: the gap is 3 (10 - 0.5) = 28.5 up to the posterior's own 0.01."""
    V, c = 10, 10.0
    full = [1, 2, 3, 4, 5, 6, 7, 8]
    z = torch.zeros(1, 24, V, dtype=torch.float64)
    for i, l in enumerate(full):
        z[0, 3 * i, l] = c
        z[0, 3 * i + 1, 0] = z[0, 3 * i + 2, 0] = c
    partial = full[:3] + full[6:]
    ctc_full, ctc_part = float(_ctc(z, [24], [full])), float(_ctc(z, [24], [partial]))
    star_full = float(R.star_ctc_nll(z, [24], [full], [-0.5])[0])
    star_part = float(R.star_ctc_nll(z, [24], [partial], [-0.5])[0])
    print("ctc_star peaked: ctc complete %.4f partial %.4f; star(-0.5) complete %.4f partial %.4f; gap %.3f"
          % (ctc_full, ctc_part, star_full, star_part, ctc_part - star_part))
    assert star_part < ctc_part and star_full <= ctc_full
    assert abs((ctc_part - star_part) - 28.5) <= 0.05
    assert star_part < 2.0 and ctc_full < 0.05


def test_abi_declares_the_three_entries():
    """include/asr_hip.h declares asr_ctc_star_ws_bytes / _loss_fwd / _loss_bwd, hip_backend.EXPORTS holds them, the library
    exports them, and the limit is the header's: at least 400 labels, 3 L + 2 states within the CTC chains' 2 * 1023 + 1."""
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_ctc_star_\w+)\s*\(", header, flags=re.M))
    want = {"asr_ctc_star_ws_bytes", "asr_ctc_star_loss_fwd", "asr_ctc_star_loss_bwd"}
    assert declared == want
    assert want <= set(hb.EXPORTS)
    lib = hb.load()
    assert all(hasattr(lib, n) for n in want)
    limit = int(re.search(r"^#define ASR_CTC_STAR_MAX_LABELS (\d+)", header, flags=re.M).group(1))
    assert limit == hb.CTC_STAR_MAX_LABELS and limit >= 400 and 3 * limit + 2 <= 2 * hb.CTC_MAX_LABELS + 1
    B, T, V, L = 3, 7, 5, 2
    assert hb.ctc_star_ws_bytes(B, T, V, L) >= 4 * (B * T * (3 * L + 4) + B * (L + V + 1))
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_star_ws_bytes(2, 10, 5, limit + 1)
    with pytest.raises(hb.UnsupportedShape):
        hb.ctc_star_ws_bytes(2, 10, 1, 3)


def test_model_arguments():
    """E2E(ctc_star_penalty): absent -> None; it needs the CTC branch; a positive value is refused; no parameter and no
    state_dict key comes with it."""
    import __graft_entry__ as entry
    entry.build()
    import model as M
    import synth
    kw = dict(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY)
    plain = M.E2E(ctc_weight=0.3, **kw)
    star = M.E2E(ctc_weight=0.3, ctc_star_penalty=-0.5, **kw)
    assert plain.ctc_star_penalty is None and star.ctc_star_penalty == -0.5
    assert list(plain.state_dict()) == list(star.state_dict())
    with pytest.raises(ValueError):
        M.E2E(ctc_star_penalty=-0.5, **kw)
    with pytest.raises(ValueError):
        M.E2E(ctc_weight=0.3, ctc_star_penalty=0.5, **kw)

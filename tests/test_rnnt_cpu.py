"""The transducer head without a GPU: the float64 restatement (tests/rnnt_ref.py) against path enumeration and central
differences, the model's and the solver's argument checks, the exports, the shapes the library refuses, and the top-two
logit margin of the decode inputs the GPU tests use."""
import os
import re

import numpy as np
import pytest
import torch

import rnnt_ref as R
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(T, U, V, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-2, 2, (T, U + 1, V)), rs.randint(1, V, U)


def test_float64_loss_is_the_sum_over_all_paths():
    n = 0
    for T in range(1, 5):
        for U in range(0, 4):
            for V in range(2, 5):
                z, y = _case(T, U, V, 100 * T + 10 * U + V)
                got, want = float(R.loss_and_grad(z, y)[0]), float(R.brute_force_nll(z, y))
                assert abs(got - want) <= 1e-12 * abs(want), (T, U, V, got, want)
                assert abs(float(R.torch_nll(torch.from_numpy(z), y)) - want) <= 1e-12 * abs(want), (T, U, V)
                n += 1
    assert n == 48


@pytest.mark.parametrize("T,U,V", [(1, 0, 2), (1, 2, 3), (3, 0, 4), (4, 3, 4), (2, 5, 3)])
def test_analytic_gradient_equals_central_differences(T, U, V):
    """float64 central differences with h = 1e-5: truncation ~ h^2 |f'''| ~ 1e-10, rounding ~ eps |f| / h ~ 1e-10."""
    z, y = _case(T, U, V, 7 + T + U + V)
    _, grad = R.loss_and_grad(z, y, g=0.75)
    h = 1e-5
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        fd = 0.75 * (float(R.loss_and_grad(zp, y)[0]) - float(R.loss_and_grad(zm, y)[0])) / (2 * h)
        assert abs(fd - grad[idx]) <= 1e-8, (idx, fd, grad[idx])
    t = torch.from_numpy(z).requires_grad_()
    (0.75 * R.torch_nll(t, y)).backward()
    assert np.abs(t.grad.numpy() - grad).max() <= 1e-12


def test_joint_backward_is_the_gradient_of_the_joint():
    rs = np.random.RandomState(3)
    pe, pp, dz = rs.uniform(-1, 1, (3, 4)), rs.uniform(-1, 1, (5, 4)), rs.uniform(-1, 1, (3, 5, 4))
    a, b = torch.from_numpy(pe).requires_grad_(), torch.from_numpy(pp).requires_grad_()
    z = torch.tanh(a[:, None] + b[None])
    assert np.abs(z.detach().numpy() - R.joint(pe, pp)).max() <= 1e-15
    (z * torch.from_numpy(dz)).sum().backward()
    dpe, dpp = R.joint_bwd(dz, R.joint(pe, pp))
    assert np.abs(a.grad.numpy() - dpe).max() <= 1e-14 and np.abs(b.grad.numpy() - dpp).max() <= 1e-14


def _e2e(**kw):
    import model as M
    return M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY, **kw)


def test_weight_zero_is_the_parent_model():
    plain, off = _e2e(), _e2e(rnnt_weight=0.0, rnnt_joint_dim=32, rnnt_pred_dim=8)
    assert list(off.state_dict()) == list(plain.state_dict()) and set(plain.state_dict()) == set(synth.e2e_weights(synth.TINY, 11))
    assert not hasattr(off, "rnnt")
    on = _e2e(rnnt_weight=0.5, ctc_weight=0.2, rnnt_joint_dim=32)
    extra = sorted(set(on.state_dict()) - set(plain.state_dict()))
    assert extra == sorted(["ctc_lo.weight", "ctc_lo.bias"] + ["rnnt." + k for k in R.HEAD_KEYS]), extra
    assert on.rnnt.lstm.weight_hh_l0.shape == (4 * synth.TINY["dec_hidden_dim"], synth.TINY["dec_hidden_dim"])
    assert _e2e(rnnt_weight=0.5, rnnt_joint_dim=8, rnnt_pred_dim=12).rnnt.lin_pred.weight.shape == (8, 12)


def test_weight_checks_raise():
    for kw in (dict(rnnt_weight=-0.1), dict(rnnt_weight=1.5), dict(rnnt_weight=0.6, ctc_weight=0.5),
               dict(rnnt_weight=0.3, pad=3), dict(rnnt_weight=0.3, rnnt_joint_dim=30)):
        with pytest.raises(ValueError):
            _e2e(**kw)
    _e2e(rnnt_weight=0.5, ctc_weight=0.5, rnnt_joint_dim=32)
    with pytest.raises(ValueError):
        _e2e().rnnt_nll(None, None)
    with pytest.raises(ValueError):
        _e2e().recognize_rnnt(torch.zeros(1, 4, 8), [4])


def test_solver_key_checks_raise():
    from solver import Solver
    assert Solver.rnnt_model_args({}) == {} and Solver.rnnt_model_args(dict(rnnt_weight=0, rnnt_joint_dim=64)) == {}
    assert Solver.rnnt_model_args(dict(rnnt_weight=0.3)) == dict(rnnt_weight=0.3, rnnt_joint_dim=256, rnnt_pred_dim=None)
    with pytest.raises(ValueError):
        Solver.rnnt_model_args(dict(rnnt_weight=0.7, ctc_weight=0.4))
    assert Solver.rnnt_decode_config({}, False) is False
    assert Solver.rnnt_decode_config(dict(rnnt_greedy_decode=True, beam_size=1), True) is True
    with pytest.raises(ValueError, match="rnnt_weight"):
        Solver.rnnt_decode_config(dict(rnnt_greedy_decode=True), False)
    for other in (dict(beam_size=4), dict(lm_weight=0.2), dict(ctc_decode_weight=0.3), dict(two_pass_decode=True),
                  dict(ctc_beam_decode=True), dict(ctc_greedy_decode=True), dict(ngram_lm="lm.arpa"), dict(word_lm="w.arpa")):
        with pytest.raises(ValueError, match="does not combine"):
            Solver.rnnt_decode_config(dict(rnnt_greedy_decode=True, **other), True)


def test_joint_loss_combines_the_three_terms():
    import parallel
    att = torch.tensor(2.0)
    lp = torch.zeros(2, 3)
    lp.ctc_loss, lp.ctc_weight, lp.ctc_norm = torch.tensor(5.0), 0.2, 4.0
    assert float(parallel.joint_loss(att, lp, dict(b_global=4))) == pytest.approx(0.8 * 2 + 0.2 * 5)
    lp.rnnt_loss, lp.rnnt_weight, lp.rnnt_norm = torch.tensor(7.0), 0.5, 2.0
    want = 0.3 * 2 + 0.2 * 5 + 0.5 * 7 * (2.0 / 4.0)                # (the rnnt term was divided by 2 utterances, 4 are global)
    assert float(parallel.joint_loss(att, lp, dict(b_global=4))) == pytest.approx(want)
    only = torch.zeros(2, 3)
    only.rnnt_loss, only.rnnt_weight, only.rnnt_norm = torch.tensor(7.0), 0.5, 4.0
    assert float(parallel.joint_loss(att, only, dict(b_global=4))) == pytest.approx(0.5 * 2 + 0.5 * 7)


NEW_EXPORTS = ("asr_rnnt_ws_bytes", "asr_rnnt_joint_fwd_f32", "asr_rnnt_joint_bwd_f32", "asr_rnnt_loss_fwd_f32",
               "asr_rnnt_loss_bwd_f32", "asr_rnnt_greedy_step_f32")


def test_exports_are_declared():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    declared = set(re.findall(r"^int\s+(asr_rnnt_\w+)\s*\(", header, flags=re.M))
    assert declared == set(NEW_EXPORTS) and declared <= set(hb.EXPORTS)
    assert "LOWER INDEX ON TIES" in header
    lib = hb.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name


def test_refused_shapes():
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    words = hb.rnnt_ws_bytes(32, 100, 100, 256, 34)
    assert words >= 4 * (3 * 32 * 100 * 101 + 32)
    for B, T, U, J, V in ((2, 5, 3, 8, 1),               # V < 2
                          (2, 5, 3, 6, 5),               # J not a multiple of 4
                          (2, 5, hb.RNNT_MAX_LABELS + 1, 8, 5),
                          (1 << 15, 1 << 15, 1000, 256, 34),       # 2^40 nodes: beyond the launch grids
                          (1 << 12, 1 << 12, 1000, 1 << 20, 34)):  # 2^24 nodes of 2^20 units: beyond 2^40 elements
        with pytest.raises(hb.UnsupportedShape):
            hb.rnnt_ws_bytes(B, T, U, J, V)
    with pytest.raises(RuntimeError):
        hb.rnnt_ws_bytes(0, 5, 3, 8, 5)


@pytest.mark.parametrize("name", sorted(R.DECODE_CASES))
def test_decode_inputs_have_a_margin(name):
    """Every step of the float64 greedy on the GPU tests' decode inputs separates its two best logits by at least 1e-3 -
    three orders of magnitude above the fp32 error of a J = 32 dot product of O(1) terms (32 x 2^-24 ~ 2e-6) - so the fp32
    kernels must choose the same tokens, and the float32 restatement does.  The cases cover what their names promise."""
    p, enc_h, lens, max_symbols, max_len = R.decode_case(name)
    rows = [R.greedy(p, enc_h[b, :n], 1, max_symbols, max_len) for b, n in enumerate(lens)]
    for b, r in enumerate(rows):
        assert r["margin"] >= 1e-3, (name, b, r["margin"])
        r32 = R.greedy(p, enc_h[b, :lens[b]], 1, max_symbols, max_len, dt=np.float32)
        assert r32["tokens"] == r["tokens"], (name, b)
    assert 1 in lens
    if name == "mixed":
        assert len(set(r["iterations"] for r in rows)) > 1, [r["iterations"] for r in rows]
        assert any(r["tokens"] for r in rows)
    else:
        assert any(r["hit_max"] for r in rows) and any(r["hit_cap"] for r in rows)

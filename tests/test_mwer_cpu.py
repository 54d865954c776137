"""MWER training without a GPU: the float64 restatement of the loss (tests/mwer_ref.py) against central finite differences
and its invariances, the float32 restatement beside it, the two C entries (declared, exported, their argument errors - they
answer before anything is launched), the config keys, and the learning rate of the GPU descent test on the float64 oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import mwer_ref as R
import synth

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(B=2, K=3, L=4, V=5, seed=0):
    rs = np.random.RandomState(seed)
    return dict(B=B, logits=rs.normal(0, 1.5, size=(L, B * K, V)), tokens=rs.randint(0, V, size=(L, B * K)),
                npos=rs.randint(1, L + 1, size=B * K), err=rs.randint(0, 6, size=B * K), scale=1.0 / B)


def _run(c, g=1.0):
    return R.run_f64(c["logits"], c["tokens"], c["npos"], c["err"], c["B"], c["scale"], g)


def test_gradient_against_central_differences():
    c = _small()
    c["err"] = np.array([0, 3, 1, 2, 2, 5])
    out = _run(c)
    assert abs(out["loss"]) > 1e-3 and np.abs(out["dlogits"]).max() > 1e-3
    h = 1e-6
    num = np.zeros_like(c["logits"])
    for i in np.ndindex(*c["logits"].shape):
        for sgn in (1, -1):
            z = c["logits"].copy()
            z[i] += sgn * h
            num[i] += sgn * float(R.run_f64(z, c["tokens"], c["npos"], c["err"], c["B"], c["scale"])["loss"])
    num /= 2 * h
    assert np.abs(num - out["dlogits"]).max() <= 1e-8 * max(1.0, np.abs(out["dlogits"]).max())
    # the closed form the kernel uses: coef = d risk_b / d s_r, dlogits = g scale coef (onehot - softmax) on the scored positions
    soft = torch.softmax(torch.from_numpy(c["logits"]), -1).numpy()
    onehot = np.zeros_like(soft)
    np.put_along_axis(onehot, c["tokens"][..., None], 1.0, -1)
    closed = c["scale"] * out["coef"][None, :, None] * (onehot - soft)
    closed[np.arange(4)[:, None] >= c["npos"][None, :]] = 0
    assert np.abs(closed - out["dlogits"]).max() <= 1e-14


def test_float32_restatement_follows_the_float64_one():
    for c in (R.make_case(g) for g in R.GRID[:4]):
        a = R.run_f64(c["logits"], c["tokens"], c["npos"], c["err"], c["B"], c["scale"], c["g"])
        b = R.run_f32(c["logits"], c["tokens"], c["npos"], c["err"], c["B"], c["scale"], c["g"])
        for k in ("loss", "risk", "post", "seq_logp", "coef", "dlogits"):
            scale = max(1.0, float(np.abs(a[k]).max())) if a[k].size else 1.0
            assert np.abs(a[k] - b[k]).max() <= 2e-4 * scale, k


def test_one_hypothesis_or_equal_errors_give_zero():
    c = _small(K=1)
    out = _run(c)
    assert out["loss"] == 0 and not out["dlogits"].any() and (out["post"] == 1).all()
    c = _small()
    c["err"] = np.array([4, 4, 4, 1, 1, 1])
    out = _run(c)
    assert abs(out["loss"]) <= 1e-16 and np.abs(out["dlogits"]).max() <= 1e-16 and not out["risk"].any()
    f32 = R.run_f32(c["logits"], c["tokens"], c["npos"], c["err"], c["B"], c["scale"])
    assert f32["loss"] == 0 and not f32["dlogits"].any()


def test_unused_slots_change_nothing():
    c = _small()
    base = _run(c)
    L, Rr, V = c["logits"].shape
    # K = 3 -> 5: an unused slot in the middle and one at the end of every utterance, holding other logits and errors
    keep = np.array([0, 2, 3, 5, 7, 8])
    rs = np.random.RandomState(9)
    z = rs.normal(0, 5, size=(L, 10, V))
    z[:, keep] = c["logits"]
    tokens = rs.randint(0, V, size=(L, 10))
    tokens[:, keep] = c["tokens"]
    npos, err = np.array([0, 0, 0, 0, -1] * 2), rs.randint(0, 50, size=10)
    npos[keep], err[keep] = c["npos"], c["err"]
    out = R.run_f64(z, tokens, npos, err, 2, c["scale"])
    assert out["loss"] == base["loss"] and (out["risk"] == base["risk"]).all()
    assert (out["dlogits"][:, keep] == base["dlogits"]).all() and (out["post"][keep] == base["post"]).all()
    gone = np.setdiff1d(np.arange(10), keep)
    assert not out["dlogits"][:, gone].any() and not out["post"][gone].any() and not out["coef"][gone].any()
    assert not out["seq_logp"][gone].any()
    # an utterance without a live slot: risk 0, and the other utterance's numbers stay
    npos2 = npos.copy()
    npos2[5:] = 0
    out2 = R.run_f64(z, tokens, npos2, err, 2, c["scale"])
    assert out2["risk"][1] == 0 and out2["risk"][0] == base["risk"][0] and not out2["dlogits"][:, 5:].any()
    f32 = R.run_f32(z, tokens, npos2, err, 2, c["scale"])
    assert f32["risk"][1] == 0 and not f32["dlogits"][:, 5:].any() and not f32["dlogits"][:, gone].any()


def test_a_constant_added_to_an_utterances_errors_changes_nothing():
    c = _small()
    base = _run(c)
    c2 = dict(c, err=c["err"] + np.array([7, 7, 7, 0, 0, 0]))
    out = _run(c2)
    assert abs(out["loss"] - base["loss"]) <= 1e-14 and np.abs(out["dlogits"] - base["dlogits"]).max() <= 1e-14


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert re.search(r"^int asr_mwer_fwd_f32\(int B, int K, int L, int V, const float\* logits, int64_t ld, "
                     r"const int64_t\* tokens,", header, flags=re.M)
    assert re.search(r"^int asr_mwer_bwd_f32\(int B, int K, int L, int V, const float\* logits, int64_t ld, "
                     r"const int64_t\* tokens,", header, flags=re.M)
    assert re.search(r"#define ASR_ABI_VERSION 8\b", header)
    entry.build()
    import hip_backend as hb
    assert "asr_mwer_fwd_f32" in hb.EXPORTS and "asr_mwer_bwd_f32" in hb.EXPORTS and hb.ABI_VERSION == 8
    lib = hb.load()
    assert hasattr(lib, "asr_mwer_fwd_f32") and hasattr(lib, "asr_mwer_bwd_f32")


def test_argument_errors_come_back_before_any_launch():
    """Both entries look at their arguments first: with a null pointer, a non-positive size or a beam above ASR_BEAM_KMAX
    they return before they touch the device (the pointers below are never dereferenced)."""
    entry.build()
    import hip_backend as hb
    lib = hb.load()
    p, null = ctypes.c_void_p(4096), None
    E_ARG, E_SHAPE = -1, -2

    def fwd(B=2, K=4, L=3, V=5, ld=5, logits=p, tokens=p, npos=p, err=p, outs=(p,) * 5, ws=p, ws_bytes=1 << 20):
        return lib.asr_mwer_fwd_f32(B, K, L, V, logits, ld, tokens, npos, err, 0.5, *outs, ws, ws_bytes, None)

    def bwd(B=2, K=4, L=3, V=5, ld=5, logits=p, tokens=p, npos=p, coef=p, g=p, dz=p, lddz=5):
        return lib.asr_mwer_bwd_f32(B, K, L, V, logits, ld, tokens, npos, coef, g, 0.5, dz, lddz, None)
    for kw in (dict(B=0), dict(K=0), dict(L=0), dict(V=0), dict(B=-1), dict(ld=4), dict(logits=null), dict(tokens=null),
               dict(npos=null), dict(err=null), dict(ws=null), dict(ws_bytes=4 * 2 * 4 * 3 - 1)):
        assert fwd(**kw) == E_ARG, kw
    for i in range(5):
        assert fwd(outs=tuple(null if j == i else p for j in range(5))) == E_ARG, i
    for kw in (dict(B=0), dict(K=0), dict(L=0), dict(V=0), dict(ld=4), dict(lddz=4), dict(logits=null), dict(tokens=null),
               dict(npos=null), dict(coef=null), dict(g=null), dict(dz=null)):
        assert bwd(**kw) == E_ARG, kw
    assert fwd(K=hb.BEAM_KMAX + 1) == E_SHAPE and bwd(K=hb.BEAM_KMAX + 1) == E_SHAPE
    assert fwd(B=1 << 27, K=16, L=1 << 10, ws_bytes=1 << 62) == E_SHAPE            # more (l, r) rows than a grid holds


def test_config_keys():
    with open(os.path.join(ROOT, "semi-supervised-asr_amd", "config.yaml")) as f:
        text = f.read()
    base = yaml.safe_load(text)
    for key in ("mwer_beam", "mwer_ce_weight", "mwer_epochs"):
        assert key not in base and ("# %s:" % key) in text                          # present, commented out: off
    entry.build()
    from solver import Solver
    assert Solver.mwer_config(base) is None and Solver.mwer_config(dict(mwer_ce_weight=0.5)) is None
    assert Solver.mwer_config(dict(mwer_beam=4)) == (4, 0.01, 1)
    assert Solver.mwer_config(dict(mwer_beam=16, mwer_ce_weight=0.0, mwer_epochs=3)) == (16, 0.0, 3)
    for bad in (dict(mwer_beam=1), dict(mwer_beam=17), dict(mwer_beam=4, mwer_ce_weight=-1.0), dict(mwer_beam=4, mwer_epochs=0)):
        with pytest.raises(ValueError):
            Solver.mwer_config(bad)
    with pytest.raises(ValueError, match="one process"):
        Solver.mwer_config(dict(mwer_beam=4), world=2)
    main = open(os.path.join(ROOT, "semi-supervised-asr_amd", "main.py")).read()
    assert '"--mwer_train"' in main and "solver.mwer_train()" in main


def test_the_descent_tests_learning_rate_on_the_float64_oracle():
    """What tests/test_mwer_gpu.py asks of ten Solver.mwer_train_one_iteration steps - frozen hypotheses, dropout 0, a lower
    mean risk at the end - holds for the float64 oracle alone at R.DESCENT_LR: Adam with the Solver's settings, clipped."""
    from oracle import asr_oracle as O
    cfg = dict(synth.TINY)
    ld = synth.labeldist(cfg["output_dim"], 12)
    weights = synth.e2e_weights(cfg, 11)
    xs, ilens, ys = synth.batch(cfg["input_dim"], cfg["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    sd = {k: v.detach().double().requires_grad_() for k, v in O.make_leaf_state(weights).items()
          if not k.startswith("decoder.attention.")}
    for k in list(sd):
        if k.startswith("attention."):
            sd["decoder." + k] = sd[k]
    tokens, lengths = R.fixed_hyps(ys, 4, cfg["output_dim"], 2)
    names = O.unique_param_names(sd)
    opt = O.AdamAmsgrad(names, lr=R.DESCENT_LR, weight_decay=1e-6)
    ys_t = [torch.from_numpy(y) for y in ys]
    risks = []
    for _ in range(R.DESCENT_STEPS + 1):
        np.random.seed(0)
        loss, risk = R.oracle_step_loss(O, sd, dict(cfg, labeldist=ld), torch.from_numpy(xs).double(), ilens, ys_t, tokens,
                                        lengths, 0.01)
        risks.append(risk)
        grads = torch.autograd.grad(loss, [sd[n] for n in names])
        clipped, _ = O.clip_global_norm(list(grads), 5.0)
        opt.step(sd, dict(zip(names, clipped)))
    print("mean risk over the steps:", " ".join("%.5f" % r for r in risks))
    assert risks[-1] < risks[0] - 1e-3 and risks[0] != 0

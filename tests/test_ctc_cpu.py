"""Host side of the CTC branch, no GPU: the rank-local joint losses of parallel.sup_local_loss sum to the single-process
joint loss, and Solver.build_model creates the head exactly when `ctc_weight` > 0."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, D, W = 7, 5, 0.3


def _stand_in(use_loss_norm):
    """E2E.forward's signature and its contract with parallel.local_loss, in float64 on the CPU: log-probs [b, olength] (any
    fixed function of the utterance), and on them the CTC term as E2E attaches it - ctc_loss = sum of this shard's
    per-utterance nll / ctc_norm, ctc_norm, ctc_weight - with torch's ctc_loss as the nll."""
    proj = torch.from_numpy(np.random.RandomState(3).normal(0, 1, size=(D, V)))

    def fwd(xs, ilens, ys, tf_rate=1.0, sample=False, total_length=None, olength=None, loss_norm=None):
        assert (loss_norm is not None) == use_loss_norm and xs.shape[1] == total_length[0]
        logits = xs @ proj                                                    # [b, T, V]
        lp = -torch.stack([(logits[i, :n].mean() ** 2 + torch.arange(olength, dtype=torch.float64) * 0.1 * n)
                           for i, n in enumerate(ilens)])
        nll = F.ctc_loss(F.log_softmax(logits, -1).transpose(0, 1), torch.cat(ys), torch.tensor(ilens),
                         torch.tensor([len(y) for y in ys]), blank=0, reduction="none", zero_infinity=True)
        norm = float(loss_norm) if loss_norm else float(len(ys))
        lp.ctc_nll, lp.ctc_loss, lp.ctc_norm, lp.ctc_weight = nll, nll.sum() / norm, norm, W
        return None, lp, None, None
    fwd.accepts_loss_norm = use_loss_norm
    return fwd


@pytest.mark.parametrize("use_loss_norm", [True, False])
@pytest.mark.parametrize("world", [2, 3])
def test_shard_losses_sum_to_the_joint_loss(world, use_loss_norm):
    import parallel
    rs = np.random.RandomState(11)
    for ilens in ([9, 8, 6, 5, 4], [7, 6]):                                   # 2 utterances on 3 ranks: an empty shard
        B = len(ilens)
        xs = torch.zeros(B, max(ilens), D, dtype=torch.float64)
        for i, n in enumerate(ilens):
            xs[i, :n] = torch.from_numpy(rs.normal(0, 1, size=(n, D)))
        ys = [torch.from_numpy(rs.randint(1, V, size=(m,))) for m in ([3, 2, 4, 1, 2][:B])]
        fwd = _stand_in(use_loss_norm)
        np.random.seed(0)
        whole = parallel.sup_local_loss(fwd, xs, ilens, ys, 1.0, 0, 1, 0, [])
        # the single-process joint loss, written out
        _, lp, _, _ = fwd(xs, ilens, ys, total_length=[max(ilens)], olength=max(len(y) for y in ys) + 1,
                          **(dict(loss_norm=B) if use_loss_norm else {}))
        want = (1 - W) * (-lp.sum() / (B * lp.shape[1])) + W * lp.ctc_nll.sum() / B
        assert float(lp.ctc_nll.min()) > 0
        assert abs(float(whole) - float(want)) <= 1e-12 * abs(float(want))
        parts = [parallel.sup_local_loss(fwd, xs, ilens, ys, 1.0, r, world, 0, []) for r in range(world)]
        assert [p is None for p in parts] == [r >= B for r in range(world)]
        total = sum(float(p) for p in parts if p is not None)
        assert abs(total - float(want)) <= 1e-12 * abs(float(want)), (total, float(want))


def test_build_model_creates_the_head_only_when_asked(tmp_path, monkeypatch):
    from solver import Solver
    root = str(tmp_path)
    synth.write_solver_run_corpus(root, sizes=synth.SOLVER_LOOPS["corpus"])
    with open(os.path.join(ROOT, "semi-supervised-asr_amd", "config.yaml")) as f:
        base = yaml.safe_load(f)
    assert "ctc_weight" not in base                                           # not a reference key
    monkeypatch.chdir(root)
    names = {}
    for key, over in (("absent", {}), ("zero", dict(ctc_weight=0.0)), ("on", dict(ctc_weight=0.3))):
        s = Solver(synth.solver_run_config(base, root, **synth.SOLVER_LOOPS["config"], **over))
        names[key] = [n for n, _ in s.model.named_parameters()]
        assert s.model.ctc_weight == over.get("ctc_weight", 0.0)
        assert sum(p.numel() for p in s.gen_opt.buf.params) == sum(p.numel() for p in s.model.parameters())
    assert names["absent"] == names["zero"] and not any(n.startswith("ctc_lo") for n in names["zero"])
    assert names["on"] == names["zero"] + ["ctc_lo.weight", "ctc_lo.bias"]
    model_cfg, _ = synth.solver_run_model_cfg(s.config)
    assert tuple(s.model.ctc_lo.weight.shape) == (model_cfg["output_dim"], model_cfg["enc_hidden_dim"])

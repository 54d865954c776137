"""What MWER training costs.  Every measurement alternates its sides in one process behind warm-up, in windows
bracketed by device events that end in a synchronise; medians and spreads (max - min over the median) of the windows, as
tools/two_pass_bench.py takes them.

  loss   ops.mwer_loss forward + backward (3 launches) against the same loss composed from existing parts - ops.label_logprob,
         then torch where / sum / softmax / mul with autograd - on random logits [L, B K, V] at B = 32, K in {4, 8}, L = 100,
         V = 50, the lengths ragged.  The two sides' loss and gradient are compared first.
  step   Solver.mwer_train_one_iteration at cfg-2 (bench.py's model, batch 32, 800 frames, dropout 0.3) with K = 4 beside
         Solver.sup_train_one_iteration on the same batch, and the MWER step's parts timed on their own between device events:
         the n-best search, the edit distances, the scoring pass with the risk loss and its backward (from the encoder output
         on); `rest` = the step minus these: the encoder both ways, the cross-entropy pass, clip + Adam.

Appends its JSON lines to profiles/mwer_bench.jsonl."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _alternate(sides, rounds, calls, warmup):
    windows = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            for _ in range(warmup):
                fn()
            windows[name].append(_window(fn, calls))
    med = {k: statistics.median(w) for k, w in windows.items()}
    spread = {k: (max(w) - min(w)) / med[k] for k, w in windows.items()}
    return windows, med, spread


def _composed(ops, logits, tok_lb, npos, err, B):
    L, R, _ = logits.shape
    K = R // B
    logp = ops.label_logprob(logits, tok_lb)
    mask = torch.arange(L, device=logits.device).unsqueeze(1) < npos.unsqueeze(0)
    s = torch.where(mask, logp, torch.zeros((), device=logits.device)).sum(0).view(B, K)
    post = torch.softmax(s, dim=1)
    e = err.view(B, K).float()
    return (post * (e - e.mean(1, keepdim=True))).sum(1).sum() / B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="calls per window of the loss alone")
    ap.add_argument("--step-calls", type=int, default=5, help="calls per window of a train step or one of its parts")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mwer_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import hip_backend as hb
    import ops
    import synth
    assert torch.cuda.is_available(), "mwer_bench.py measures on the GPU"
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    r4 = lambda x: round(x, 4)                                                                  # noqa: E731

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    B, L, V = 32, 100, 50
    for K in (4, 8):
        R = B * K
        rs = np.random.RandomState(K)
        logits = torch.from_numpy((3.0 * rs.normal(0, 1, size=(L, R, V))).astype(np.float32)).to(dev).requires_grad_()
        # neighbouring hypotheses: the scores of a list lie within a few nats, so the posteriors are not saturated
        tok_b = rs.randint(3, V, size=(L, B, 1)).repeat(K, 2)
        flip = rs.uniform(size=(L, B, K)) < 0.05
        tok = torch.from_numpy(np.where(flip, rs.randint(3, V, size=(L, B, K)), tok_b).reshape(L, R)).to(dev)
        with torch.no_grad():
            logits[:, :, :].scatter_add_(2, tok.unsqueeze(2), torch.full((L, R, 1), 9.0, device=dev))
        npos = torch.from_numpy((L - (np.arange(R) * 7) % 40).astype(np.int32)).to(dev)
        err = torch.from_numpy(rs.randint(0, 20, size=R).astype(np.int32)).to(dev)

        def fused():
            logits.grad = None
            loss, _ = ops.mwer_loss(logits, tok, npos, err, 1.0 / B)
            loss.backward()
            return loss

        def composed():
            logits.grad = None
            loss = _composed(ops, logits, tok, npos, err, B)
            loss.backward()
            return loss
        la = fused()
        ga = logits.grad.clone()
        lb = composed()
        gb = logits.grad.clone()
        torch.cuda.synchronize()
        gscale = float(gb.abs().max())
        assert gscale > 0 and abs(float(la) - float(lb)) <= 1e-4 * max(1.0, abs(float(lb)))
        assert float((ga - gb).abs().max()) <= 1e-3 * gscale
        w, m, s = _alternate((("fused", fused), ("composed", composed)), args.rounds, args.calls, args.warmup)
        emit(dict(tool="tools/mwer_bench.py", what="loss fwd+bwd", B=B, K=K, L=L, V=V, rounds=args.rounds,
                  calls_per_window=args.calls, ms_fused=r4(m["fused"]), ms_composed=r4(m["composed"]),
                  ratio_composed_over_fused=round(m["composed"] / m["fused"], 3), spread_fused=r4(s["fused"]),
                  spread_composed=r4(s["composed"]), windows_ms_fused=[r4(x) for x in w["fused"]],
                  windows_ms_composed=[r4(x) for x in w["composed"]], loss=float(la), max_grad=gscale,
                  max_grad_difference=float((ga - gb).abs().max()), launches_fused=3))
    if args.skip_step:
        return

    import bench
    K = 4
    spec = bench.CONFIGS["cfg2"]
    cfg = dict(spec["model"])
    torch.manual_seed(1000)
    np.random.seed(1000)
    solver = bench.make_solver(cfg, spec["batch"], spec["frames"], os.path.join(tempfile.mkdtemp(prefix="mwer_bench_"), "main"),
                               mwer_beam=K, mwer_ce_weight=0.01)
    xs, lens, ys = synth.ragged_batch(spec["batch"], spec["frames"], cfg["input_dim"], cfg["output_dim"], 1234)
    xs_d = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
    ys_d = [torch.from_numpy(y).to(dev) for y in ys]
    net, dec = solver.model, solver.model.decoder
    Bs = len(lens)
    steps = min(int(solver.config["max_dec_timesteps"]), max(int(y.shape[0]) for y in ys) + net.MWER_EXTRA_STEPS)

    def mwer_step():
        solver.mwer_train_one_iteration(xs_d, lens, ys_d)

    def sup_step():
        solver.sup_train_one_iteration(xs_d, lens, ys_d, 1.0)
    mwer_step()
    solver.flush()
    parts = net.last_mwer
    tokens, hyp_len, errs = parts["tokens"], parts["hyp_len"], parts["err"]
    with torch.no_grad():
        enc_h, enc_lens = net.encoder(xs_d, lens)
    enc_h = enc_h.detach().requires_grad_()
    ref = dec._label_matrices(ys_d)[1].to(torch.int32).contiguous()
    ref_len = hb.to_device_i32([int(y.shape[0]) for y in ys], dev)
    ref_index = (torch.arange(Bs * K, device=dev, dtype=torch.int32) // K).int()

    def search():
        with torch.no_grad():
            dec.recognize_beams(enc_h.detach(), enc_lens, steps, K, nbest=True)

    def edit():
        hb.edit_distance(tokens.reshape(Bs * K, -1), ref, ref_len, hyp_len=hyp_len.reshape(-1).clamp(min=0),
                         ref_index=ref_index, eos=dec.eos)

    def scoring():
        net.zero_grad()
        enc_h.grad = None
        _, logits, tok_lb, npos = dec.score_hypotheses_grad(enc_h, enc_lens, tokens, hyp_len, scores=False)
        loss, _ = ops.mwer_loss(logits, tok_lb, npos, errs, 1.0 / Bs)
        loss.backward()

    def flushed(fn):
        def run():
            fn()
            solver.flush()
        return run
    hb.LAUNCHES.clear()
    search()
    search_steps = hb.LAUNCHES["beam_step"]
    sides = (("mwer_step", flushed(mwer_step)), ("sup_step", flushed(sup_step)), ("search", search), ("edit_distance", edit),
             ("scoring_fwd_bwd", scoring))
    w, m, s = _alternate(sides, args.rounds, args.step_calls, args.warmup)
    rest = m["mwer_step"] - m["search"] - m["edit_distance"] - m["scoring_fwd_bwd"]
    emit(dict(tool="tools/mwer_bench.py", what="train step", config="cfg2", B=Bs, K=K, frames=spec["frames"],
              search_steps=search_steps, hyp_columns=int(tokens.shape[2]), live_share_of_slots=r4(float((hyp_len >= 0).float().mean())),
              rounds=args.rounds, calls_per_window=args.step_calls,
              ms_mwer_step=r4(m["mwer_step"]), ms_sup_step=r4(m["sup_step"]),
              ratio_mwer_over_sup=round(m["mwer_step"] / m["sup_step"], 3), ms_search=r4(m["search"]),
              ms_edit_distance=r4(m["edit_distance"]), ms_scoring_fwd_bwd=r4(m["scoring_fwd_bwd"]), ms_rest=r4(rest),
              spread={k: r4(v) for k, v in s.items()}, windows_ms={k: [r4(x) for x in v] for k, v in w.items()}))


if __name__ == "__main__":
    main()

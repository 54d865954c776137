"""What the graph CTC loss costs, three measurements, each ALTERNATING its sides in one process behind warm-up:

  lattice  ops.gtc_loss forward + backward on gtc.Graph.ctc graphs against ops.ctc_loss forward + backward of the same tree
           on the same rows, at B = 32, T' = 100, V = 34 with ragged frame lengths and ragged label counts up to 40.
  nbest    ops.gtc_loss on the K = 8 prefix trees of real ops.ctc_beam output at the same shape against the composition of
           8 ops.ctc_loss calls plus logsumexp, forward + backward, with the node counts of both.
  step     Solver.pseudo_train_one_iteration at cfg-2 (ctc_weight 0.3, pseudo_beam 8) against sup_train_one_iteration, and
           the pseudo step by parts: the n-best search with its host read, the graph build + compile + upload, the rest.

Each appends one JSON line to profiles/gtc_bench.jsonl.  Wall clock around windows that end in a device synchronise; the
median window of each side and the spread of each side's own windows (max - min over the median: a difference inside it is
not one)."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def _append(path, rec):
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def _spread(w, med):
    return round((max(w) - min(w)) / med, 4)


def _alternate(args, sides):
    windows = {k: [] for k in sides}
    for _ in range(args.rounds):
        for side, fn in sides.items():
            for _ in range(args.warmup):
                fn()
            windows[side].append(_window(fn, args.calls))
    return windows, {k: statistics.median(w) for k, w in windows.items()}


def _shape(hb, dev):
    B, Tp, V, lmax = 32, 100, 34, 40
    rs = np.random.RandomState(1234)
    ylens = [int(n) for n in rs.randint(8, lmax + 1, size=B)]
    ylens[0] = lmax
    flens = [int(n) for n in rs.randint(60, Tp + 1, size=B)]
    flens[0] = Tp
    flens = [max(t, 2 * n + 1) for t, n in zip(flens, ylens)]           # every utterance feasible, repeats or not
    labels = [[int(v) for v in rs.randint(1, V, size=n)] for n in ylens]
    z = (3.0 * torch.randn(B, Tp, V, generator=torch.Generator().manual_seed(5))).to(dev).requires_grad_()
    return B, Tp, V, lmax, ylens, flens, labels, z, hb.to_device_i32(flens, dev)


def bench_lattice(args, hb, ops, gtc):
    dev = torch.device("cuda")
    B, Tp, V, lmax, ylens, flens, labels, z, lens_dev = _shape(hb, dev)
    packed = torch.tensor([v for y in labels for v in y], dtype=torch.long, device=dev)
    batch = gtc.GraphBatch([gtc.Graph.ctc(y, V) for y in labels], range(B))
    table = batch.to(dev)
    g = torch.ones(B, device=dev)

    def graph():
        z.grad = None
        ops._GtcLoss.apply(z, lens_dev, table, True).backward(g)

    def plain():
        z.grad = None
        ops.ctc_loss(z, lens_dev, packed, ylens, True).backward(g)
    graph()
    plain()
    a, b = ops.gtc_loss(z.detach(), lens_dev, batch, False), ops.ctc_loss(z.detach(), lens_dev, packed, ylens, False)
    assert bool(torch.isfinite(b).all()) and float((a - b).abs().max()) <= 1e-3
    windows, med = _alternate(args, dict(gtc=graph, ctc=plain))
    _append(args.out, dict(
        tool="tools/gtc_bench.py lattice", B=B, T_out=Tp, V=V, max_label_len=lmax, mean_label_len=round(float(np.mean(ylens)), 1),
        call="forward + backward", rounds=args.rounds, calls_per_window=args.calls, ms_gtc=round(med["gtc"], 4),
        ms_ctc=round(med["ctc"], 4), ratio_gtc_over_ctc=round(med["gtc"] / med["ctc"], 3),
        windows_ms_gtc=[round(w, 4) for w in windows["gtc"]], windows_ms_ctc=[round(w, 4) for w in windows["ctc"]],
        spread_gtc=_spread(windows["gtc"], med["gtc"]), spread_ctc=_spread(windows["ctc"], med["ctc"]),
        max_nodes=table.max_nodes, max_arcs=table.max_arcs, arcs="first 4 of a node in registers, the rest from global memory",
        ws_bytes_gtc=hb.gtc_ws_bytes(B, Tp, V, table.max_nodes), ws_bytes_ctc=hb.ctc_ws_bytes(B, Tp, V, lmax)))


def bench_nbest(args, hb, ops, gtc):
    dev = torch.device("cuda")
    B, Tp, V, lmax, ylens, flens, labels, z, lens_dev = _shape(hb, dev)
    K = 8
    # logits that favour the labels, so the search returns hypotheses of their length and K distinct ones
    with torch.no_grad():
        for b, y in enumerate(labels):
            for t in range(flens[b]):
                z[b, t, y[min(t * len(y) // flens[b], len(y) - 1)] if t % 2 else 0] += 4.0
    hyp, hyp_len, score = ops.ctc_beam(z.detach(), lens_dev, K)[:3]
    hyp, hyp_len, score = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy()
    logw = gtc.nbest_weights(score, hyp_len, 1.0)
    lists = []
    for b in range(B):
        live = [k for k in range(K) if hyp_len[b, k] >= 0 and logw[b, k] > -np.inf]
        lists.append(([[int(v) for v in hyp[b, k, :hyp_len[b, k]]] for k in live], [float(logw[b, k]) for k in live]))
    assert all(len(h) == K for h, _ in lists), "the search kept fewer than K hypotheses for a row"
    graphs = [gtc.Graph.from_nbest(h, w, V) for h, w in lists]
    table = gtc.GraphBatch(graphs, range(B)).to(dev)
    g = torch.ones(B, device=dev)
    packed = [torch.tensor([v for h, _ in lists for v in h[k]], dtype=torch.long, device=dev) for k in range(K)]
    klens = [[len(h[k]) for h, _ in lists] for k in range(K)]
    wk = [torch.tensor([w[k] for _, w in lists], device=dev) for k in range(K)]

    def tree():
        z.grad = None
        ops._GtcLoss.apply(z, lens_dev, table, True).backward(g)

    def composed():
        z.grad = None
        terms = [wk[k] - ops.ctc_loss(z, lens_dev, packed[k], klens[k], False) for k in range(K)]
        (-torch.logsumexp(torch.stack(terms, 1), 1)).backward(g)
    tree()
    composed()
    windows, med = _alternate(args, dict(gtc=tree, composed=composed))
    _append(args.out, dict(
        tool="tools/gtc_bench.py nbest", B=B, T_out=Tp, V=V, K=K, call="forward + backward", rounds=args.rounds,
        calls_per_window=args.calls, ms_gtc=round(med["gtc"], 4), ms_composed=round(med["composed"], 4),
        ratio_gtc_over_composed=round(med["gtc"] / med["composed"], 3), windows_ms_gtc=[round(w, 4) for w in windows["gtc"]],
        windows_ms_composed=[round(w, 4) for w in windows["composed"]], spread_gtc=_spread(windows["gtc"], med["gtc"]),
        spread_composed=_spread(windows["composed"], med["composed"]), trie_nodes_max=table.max_nodes,
        trie_nodes_mean=round(float(np.mean([gr.N for gr in graphs])), 1),
        composed_states_max=max(2 * n + 1 for kl in klens for n in kl),
        composed_states_sum_mean=round(float(np.mean([sum(2 * klens[k][b] + 1 for k in range(K)) for b in range(B)])), 1)))


def bench_step(args, hb, synth, bench):
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp(prefix="gtc_cost_")
    spec = bench.CONFIGS["cfg2"]
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    xs, lens, ys = synth.ragged_batch(B, T, c["input_dim"], c["output_dim"], 1234)
    xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
    plain_weights = synth.e2e_weights

    def with_head(cfg, seed):                 # (bench.make_solver loads synth.e2e_weights strictly: no fixture holds a head)
        w = plain_weights(cfg, seed)
        rs = np.random.RandomState(seed + 1)
        k = 1.0 / np.sqrt(cfg["enc_hidden_dim"])
        w["ctc_lo.weight"] = rs.uniform(-k, k, size=(cfg["output_dim"], cfg["enc_hidden_dim"])).astype(np.float32)
        w["ctc_lo.bias"] = rs.uniform(-k, k, size=(cfg["output_dim"],)).astype(np.float32)
        return w
    synth.e2e_weights = with_head
    try:
        sv = bench.make_solver(c, B, T, os.path.join(tmp, "pseudo"), ctc_weight=args.ctc_weight, pseudo_beam=args.beam)
    finally:
        synth.e2e_weights = plain_weights
    K = args.beam

    def sup():
        sv.sup_train_one_iteration(xs_d, lens, ys_d, 1.0)

    def pseudo():
        sv.pseudo_train_one_iteration(xs_d, lens)

    def timed(fn, n):
        with contextlib.redirect_stdout(sys.stderr):
            for _ in range(args.warmup):
                fn()
            sv.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            sv.flush()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    windows = {"sup": [], "pseudo": []}
    for _ in range(args.rounds):
        for mode, fn in (("sup", sup), ("pseudo", pseudo)):
            windows[mode].append(timed(fn, args.steps))
    med = {m: statistics.median(w) for m, w in windows.items()}
    # the pseudo step by parts: the search with its host read, then the host's graph work, each behind a synchronise
    import gtc
    parts = {"search_and_read": [], "graphs": []}
    sv.model.eval()
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            ids, scores = sv.model.recognize_ctc_beams(xs_d, lens, K, nbest=True)
        t1 = time.perf_counter()
        score = np.full((B, K), -np.inf)
        hyp_len = np.full((B, K), -1)
        for b in range(B):
            score[b, :len(ids[b])] = scores[b]
            hyp_len[b, :len(ids[b])] = [len(h) for h in ids[b]]
        logw = gtc.nbest_weights(score, hyp_len, 1.0)
        batch = gtc.GraphBatch([gtc.Graph.from_nbest(ids[b], list(logw[b, :len(ids[b])]), c["output_dim"]) for b in range(B)], range(B))
        batch.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        parts["search_and_read"].append((t1 - t0) * 1e3)
        parts["graphs"].append((t2 - t1) * 1e3)
    sv.model.train()
    pm = {k: statistics.median(v) for k, v in parts.items()}
    _append(args.out, dict(
        tool="tools/gtc_bench.py step", config="cfg2", workload="%s, batch %d, 80x%d ragged" % (spec["name"], B, T),
        ctc_weight=args.ctc_weight, pseudo_beam=K, rounds=args.rounds, steps_per_window=args.steps,
        ms_per_step_sup=round(med["sup"], 3), ms_per_step_pseudo=round(med["pseudo"], 3),
        ratio_pseudo_over_sup=round(med["pseudo"] / med["sup"], 3), windows_ms_sup=[round(w, 3) for w in windows["sup"]],
        windows_ms_pseudo=[round(w, 3) for w in windows["pseudo"]], spread_sup=_spread(windows["sup"], med["sup"]),
        spread_pseudo=_spread(windows["pseudo"], med["pseudo"]), ms_search_and_host_read=round(pm["search_and_read"], 3),
        ms_graph_build_compile_upload=round(pm["graphs"], 3),
        ms_rest=round(med["pseudo"] - pm["search_and_read"] - pm["graphs"], 3),
        host_share=round((pm["graphs"]) / med["pseudo"], 3), mean_trie_nodes=round(float(np.mean([g.N for g in batch.graphs])), 1),
        arith=hb.arith_name()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="lattice,nbest,step")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="lattice, nbest: forward + backward calls per window")
    ap.add_argument("--steps", type=int, default=20, help="step: train steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtc_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import gtc
    import hip_backend as hb
    import ops
    import synth
    assert torch.cuda.is_available(), "gtc_bench.py measures on the GPU"
    what = args.what.split(",")
    if "lattice" in what:
        bench_lattice(args, hb, ops, gtc)
    if "nbest" in what:
        bench_nbest(args, hb, ops, gtc)
    if "step" in what:
        bench_step(args, hb, synth, bench)


if __name__ == "__main__":
    main()

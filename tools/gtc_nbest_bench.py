"""What the device-side n-best graph builder costs and saves, three measurements, each ALTERNATING its sides in
one process behind warm-up (tools/gtc_bench.py's windows, medians and spreads):

  build  ops.gtc_nbest_graphs on real ops.ctc_beam output at B = 32, K = 8, T' = 100, V = 34 against the host path on the
         same lists, already read: gtc.nbest_weights, gtc.Graph.from_nbest per row, compile, upload.
  loss   ops.gtc_loss forward + backward on the device-built table (dispatched by the bound, max_nodes 1601) against the
         host-built table of the same lists (dispatched by the largest graph).
  step   Solver.pseudo_train_one_iteration at cfg-2 (ctc_weight 0.3, pseudo_beam 8) with `pseudo_graphs_on_gpu` off and on.

Each appends one JSON line to profiles/gtc_nbest_bench.jsonl."""
import argparse
import contextlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gtc_bench as GB  # noqa: E402


def _lists(hb, ops, gtc, dev, K):
    """The shape of gtc_bench's nbest measurement: logits that favour the labels, the search's list on the device and on the
    host."""
    B, Tp, V, lmax, ylens, flens, labels, z, lens_dev = GB._shape(hb, dev)
    with torch.no_grad():
        for b, y in enumerate(labels):
            for t in range(flens[b]):
                z[b, t, y[min(t * len(y) // flens[b], len(y) - 1)] if t % 2 else 0] += 4.0
    hyp, hyp_len, score = ops.ctc_beam(z.detach(), lens_dev, K)[:3]
    host = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy()
    return B, Tp, V, z, lens_dev, (hyp, hyp_len, score), host


def _host_build(gtc, host, V, dev):
    hyp, hyp_len, score = host
    B, K = hyp_len.shape
    logw = gtc.nbest_weights(score, hyp_len, 1.0)
    graphs = []
    for b in range(B):
        live = [k for k in range(K) if logw[b, k] > -np.inf]
        graphs.append(gtc.Graph.from_nbest([[int(v) for v in hyp[b, k, :hyp_len[b, k]]] for k in live],
                                           [logw[b, k] for k in live], V))
    batch = gtc.GraphBatch(graphs, range(B))
    return batch, batch.to(dev)


def bench_build(args, hb, ops, gtc):
    dev = torch.device("cuda")
    B, Tp, V, z, lens_dev, on_dev, host = _lists(hb, ops, gtc, dev, args.beam)
    batch, _ = _host_build(gtc, host, V, dev)

    def device():
        ops.gtc_nbest_graphs(on_dev[0], on_dev[1], on_dev[2], V, 1.0)

    def on_host():
        _host_build(gtc, host, V, dev)
    windows, med = GB._alternate(args, dict(device=device, host=on_host))
    GB._append(args.out, dict(
        tool="tools/gtc_nbest_bench.py build", B=B, T_out=Tp, V=V, K=args.beam, rounds=args.rounds, calls_per_window=args.calls,
        ms_device=round(med["device"], 4), ms_host=round(med["host"], 4), ratio_device_over_host=round(med["device"] / med["host"], 4),
        windows_ms_device=[round(w, 4) for w in windows["device"]], windows_ms_host=[round(w, 4) for w in windows["host"]],
        spread_device=GB._spread(windows["device"], med["device"]), spread_host=GB._spread(windows["host"], med["host"]),
        host_side="nbest_weights + from_nbest per row + compile + upload, the list already on the host",
        mean_nodes=round(float(np.mean([g.N for g in batch.graphs])), 1), max_nodes_real=max(g.N for g in batch.graphs),
        cap_nodes=hb.gtc_nbest_bytes(B, args.beam, Tp, V)[0]))


def bench_loss(args, hb, ops, gtc):
    dev = torch.device("cuda")
    B, Tp, V, z, lens_dev, on_dev, host = _lists(hb, ops, gtc, dev, args.beam)
    batch, host_table = _host_build(gtc, host, V, dev)
    dev_table = ops.gtc_nbest_graphs(on_dev[0], on_dev[1], on_dev[2], V, 1.0)
    g = torch.ones(B, device=dev)

    def side(table):
        def run():
            z.grad = None
            ops._GtcLoss.apply(z, lens_dev, table, True).backward(g)
        return run
    a = ops.gtc_loss(z.detach(), lens_dev, dev_table, False)
    b = ops.gtc_loss(z.detach(), lens_dev, batch, False)
    assert bool(torch.isfinite(b).all()) and float((a - b).abs().max()) <= 1e-3
    windows, med = GB._alternate(args, dict(device_table=side(dev_table), host_table=side(host_table)))
    GB._append(args.out, dict(
        tool="tools/gtc_nbest_bench.py loss", B=B, T_out=Tp, V=V, K=args.beam, call="forward + backward", rounds=args.rounds,
        calls_per_window=args.calls, ms_device_table=round(med["device_table"], 4), ms_host_table=round(med["host_table"], 4),
        ratio_device_over_host=round(med["device_table"] / med["host_table"], 3),
        windows_ms_device_table=[round(w, 4) for w in windows["device_table"]],
        windows_ms_host_table=[round(w, 4) for w in windows["host_table"]],
        spread_device_table=GB._spread(windows["device_table"], med["device_table"]),
        spread_host_table=GB._spread(windows["host_table"], med["host_table"]),
        max_nodes_device_table=dev_table.max_nodes, max_nodes_host_table=host_table.max_nodes,
        ws_bytes_device_table=hb.gtc_ws_bytes(B, Tp, V, dev_table.max_nodes),
        ws_bytes_host_table=hb.gtc_ws_bytes(B, Tp, V, host_table.max_nodes), nll_bits_equal=bool(torch.equal(a, b))))


def bench_step(args, hb, synth, bench):
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp(prefix="gtc_nbest_cost_")
    spec = bench.CONFIGS["cfg2"]
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    xs, lens, _ = synth.ragged_batch(B, T, c["input_dim"], c["output_dim"], 1234)
    xs_d = torch.from_numpy(xs).to(dev)
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
        solvers = {name: bench.make_solver(c, B, T, os.path.join(tmp, name), ctc_weight=args.ctc_weight, pseudo_beam=args.beam,
                                           pseudo_graphs_on_gpu=on) for name, on in (("host", False), ("device", True))}
    finally:
        synth.e2e_weights = plain_weights

    def timed(sv, n):
        with contextlib.redirect_stdout(sys.stderr):
            for _ in range(args.warmup):
                sv.pseudo_train_one_iteration(xs_d, lens)
            sv.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                sv.pseudo_train_one_iteration(xs_d, lens)
            sv.flush()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    windows = {name: [] for name in solvers}
    for _ in range(args.rounds):
        for name, sv in solvers.items():
            windows[name].append(timed(sv, args.steps))
    med = {m: statistics.median(w) for m, w in windows.items()}
    table = solvers["device"].last_pseudo["graphs"]
    GB._append(args.out, dict(
        tool="tools/gtc_nbest_bench.py step", config="cfg2", workload="%s, batch %d, 80x%d ragged" % (spec["name"], B, T),
        ctc_weight=args.ctc_weight, pseudo_beam=args.beam, rounds=args.rounds, steps_per_window=args.steps,
        ms_per_step_host=round(med["host"], 3), ms_per_step_device=round(med["device"], 3),
        ratio_device_over_host=round(med["device"] / med["host"], 3), windows_ms_host=[round(w, 3) for w in windows["host"]],
        windows_ms_device=[round(w, 3) for w in windows["device"]], spread_host=GB._spread(windows["host"], med["host"]),
        spread_device=GB._spread(windows["device"], med["device"]), max_nodes_device_table=table.max_nodes,
        dropped=int(table.dropped.sum()), arith=hb.arith_name()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="build,loss,step")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="build, loss: calls per window")
    ap.add_argument("--steps", type=int, default=20, help="step: train steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtc_nbest_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import gtc
    import hip_backend as hb
    import ops
    import synth
    assert torch.cuda.is_available(), "gtc_nbest_bench.py measures on the GPU"
    what = args.what.split(",")
    if "build" in what:
        bench_build(args, hb, ops, gtc)
    if "loss" in what:
        bench_loss(args, hb, ops, gtc)
    if "step" in what:
        bench_step(args, hb, synth, bench)


if __name__ == "__main__":
    main()

"""What the GPU front end costs.  Two measurements, each appended as one JSON line to --out (default
profiles/frontend_bench.jsonl):

  front_end   a cfg-2 batch of waveforms (32 ragged utterances, U[0.6, 1] x 8 s of int16 at 16 kHz, 80 bins; delta_order 0
              and 2, utterance CMVN) through frontend.Frontend - samples already in HBM, device events around `--iters`
              calls - against the same computation in torch on the CPU (torch.stft-based, fp32, this machine's CPU share).
  epoch_loop  Solver.sup_train_one_iteration at cfg-2 fed by feed.DeviceFeed from waveforms (front end on the side stream)
              against the same Solver fed from precomputed features of the same frame counts, ALTERNATING in one process:
              `--rounds` rounds of (features, waveforms), each a window of `--steps` steps behind `--warmup` steps, wall
              clock around a window that ends in flush + device synchronise.  Reports the median window of either feed and
              the spread of each feed's own windows (a difference inside it is not one).

With --speed two other measurements are taken instead:

  resample    the resample launch alone (hb.resample) on the same cfg-2 waveform batch, factors 0.9 / 1.0 / 1.1 in turn over
              its rows, samples resident, device events around `--iters` calls.
  epoch_loop_speed  the cfg-2 step fed from waveforms by training feeds WITHOUT and WITH `speed_perturb: [0.9, 1.0, 1.1]`,
              alternating windows in one process as above.  The waveforms are U[0.6, 1] x 7.2 s here, so that an utterance
              slowed to 0.9 stays inside cfg-2's 800 frames; every record carries its mean frames per batch, because a
              perturbed batch is a different amount of work.

With --augment three others:

  reverb      the reverb launch alone (hb.reverb) on the same cfg-2 waveform batch, EVERY row reverberated, with RIRs of 1024
              and of 4096 taps; the achieved TFLOP/s count 2 N L flop per row (the band's 31 / L extra products not counted).
  noise_mix   the mix alone (hb.noise_mix, its two launches) on the same batch, every row mixed, in place on float32.
  epoch_loop_augment  the cfg-2 step fed from waveforms by training feeds WITHOUT and WITH `reverb` and `noise` at prob 0.5
              (synthetic banks: 8 RIRs of 4096 taps, 8 clips of 1 - 4 s), alternating windows in one process as above.
"""
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


def cpu_frontend(waves, order, threads):
    """The same computation in torch on the CPU, fp32: frames -> mean, pre-emphasis, Povey window -> torch.stft-style
    rfft power -> mel -> log -> utterance CMVN -> deltas, padded.  -> seconds per batch (best of 3)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frontend_ref as R
    torch.set_num_threads(threads)
    W = torch.from_numpy(R.mel_weights(80, 512, 16000, 20.0, 8000.0).astype(np.float32))
    window = torch.from_numpy(R.povey_window(400).astype(np.float32))
    taps = [None, torch.from_numpy(R.S1.astype(np.float32)), torch.from_numpy(R.S2.astype(np.float32))]
    xs = [torch.from_numpy(w.astype(np.float32)) for w in waves]

    def once():
        feats = []
        for x in xs:
            fr = x.unfold(0, 400, 160)
            fr = fr - fr.mean(1, keepdim=True)
            fr = (fr - 0.97 * torch.cat([fr[:, :1], fr[:, :-1]], 1)) * window
            # torch.stft on pre-cut frames: one frame per "signal", no centring, a rectangular window of n_fft
            spec = torch.stft(torch.nn.functional.pad(fr, (0, 112)), 512, hop_length=512, win_length=512, center=False,
                              window=torch.ones(512), return_complex=True)[:, :256, 0]
            logmel = torch.log(torch.clamp((spec.real ** 2 + spec.imag ** 2) @ W.T, min=R.FLT_EPSILON))
            y = (logmel - logmel.mean(0)) / logmel.var(0, unbiased=False).clamp(min=1e-10).sqrt()
            blocks = [y]
            for k in range(1, order + 1):
                w = 2 * k
                idx = (torch.arange(y.shape[0])[:, None] + torch.arange(-w, w + 1)[None, :]).clamp(0, y.shape[0] - 1)
                blocks.append((y[idx] * taps[k][None, :, None]).sum(1))
            feats.append(torch.cat(blocks, 1))
        return torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    once()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        once()
        best = min(best, time.perf_counter() - t0)
    return best


SPEEDS = [0.9, 1.0, 1.1]


def speed_lines(args, bench, hb, spec, items, samples, offs):
    """--speed: the resample launch alone, then the epoch loop without / with speed perturbation -> the records."""
    from dataset import synthetic_waveforms
    from feed import DeviceFeed
    from frontend import Frontend
    dev = samples.device
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    lines = []
    fe = Frontend(dict(n_mels=80, delta_order=0, cmvn="utterance", speed_perturb=SPEEDS))
    fidx = [b % len(SPEEDS) for b in range(B)]
    counts = [fe.perturbed_samples(b - a, f) for a, b, f in zip(offs[:-1], offs[1:], fidx)]
    out_offs = np.concatenate([[0], np.cumsum(counts)])
    offs_d, out_offs_d = hb.to_device_i64(offs, dev), hb.to_device_i64(out_offs, dev)
    fidx_d = hb.to_device_i32(fidx, dev)
    out = torch.empty(int(out_offs[-1]), device=dev)
    for _ in range(5):
        hb.resample(fe.resample_plan, samples, offs_d, fidx_d, out_offs_d, out, max_out=max(counts))
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.iters):
        hb.resample(fe.resample_plan, samples, offs_d, fidx_d, out_offs_d, out, max_out=max(counts))
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / args.iters
    moved = int(samples.numel()) * 2 + int(out.numel()) * 4
    lines.append(dict(tool="tools/frontend_bench.py", measurement="resample", factors=SPEEDS,
                      workload="%d ragged utterances, U[0.6, 1] x 8 s int16 at 16 kHz, factors in turn over the rows" % B,
                      samples_in=int(samples.numel()), samples_out=int(out.numel()), gpu_ms_per_launch=round(ms, 4),
                      bytes_moved=moved, gb_per_s=round(moved / ms / 1e6, 1),
                      timing="device events around %d launches (host enqueue included), samples resident" % args.iters))
    if args.skip_epoch_loop:
        return lines
    tmp = tempfile.mkdtemp(prefix="frontend_bench_")
    sv = bench.make_solver(c, B, T, os.path.join(tmp, "cfg2"))
    data = synthetic_waveforms(B, c["output_dim"], 7.2, seed=1234)
    short = [(v["feature"], v["token_ids"]) for v in data.values()]
    fes = {"plain": Frontend(dict(n_mels=80, delta_order=0, cmvn="utterance")), "speed_perturb": fe}
    n = args.warmup + args.steps

    def window(kind):
        feed = DeviceFeed([short] * n, dev, frontend=fes[kind], train=True)
        frames = []
        with contextlib.redirect_stdout(sys.stderr):
            for i, (xs, ilens, ys) in enumerate(feed):
                if i == args.warmup:
                    sv.flush()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if i >= args.warmup:
                    frames.append(sum(ilens))
                last = sv.sup_train_one_iteration(xs, ilens, ys, 1.0)
            sv.flush()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(np.mean(frames)), float(last)
    windows, frames, loss = {k: [] for k in fes}, {k: [] for k in fes}, {}
    np.random.seed(1234)                                  # the feeds' speed seeds
    for _ in range(args.rounds):
        for kind in fes:
            ms, fr, loss[kind] = window(kind)
            windows[kind].append(ms)
            frames[kind].append(fr)
    med = {k: statistics.median(w) for k, w in windows.items()}
    for kind in fes:
        lines.append(dict(tool="tools/frontend_bench.py", measurement="epoch_loop_speed", feed=kind,
                          call="Solver.sup_train_one_iteration",
                          workload="%s, batch %d, waveforms U[0.6, 1] x 7.2 s, training feed.DeviceFeed" % (spec["name"], B),
                          speed_perturb=SPEEDS if kind == "speed_perturb" else None, rounds=args.rounds,
                          steps_per_window=args.steps, warmup_steps=args.warmup, ms_per_step=round(med[kind], 3),
                          windows_ms=[round(w, 3) for w in windows[kind]],
                          spread=round((max(windows[kind]) - min(windows[kind])) / med[kind], 4),
                          mean_frames_per_batch=round(float(np.mean(frames[kind])), 1),
                          us_per_frame=round(med[kind] * 1e3 / float(np.mean(frames[kind])), 4),
                          over_plain=round(med[kind] / med["plain"], 4), last_loss=loss[kind], arith=hb.arith_name()))
    return lines


def _timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def _bank(clips):
    return dict(samples=np.concatenate(clips).astype(np.float32),
                offsets=np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64))


def augment_lines(args, bench, hb, spec, items, samples, offs):
    """--augment: the reverb launch alone at 1024 and 4096 taps, the mix alone, then the epoch loop without / with both."""
    from feed import DeviceFeed
    from frontend import Frontend
    dev = samples.device
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    rs = np.random.RandomState(1234)
    counts = [b - a for a, b in zip(offs[:-1], offs[1:])]
    offs_d = hb.to_device_i64(offs, dev)
    workload = "%d ragged utterances, U[0.6, 1] x 8 s int16 at 16 kHz" % B
    timing = "device events around %d calls (host enqueue included), samples resident" % args.iters
    lines = []

    def rirs(taps, n=8):
        return [rs.randn(taps) * np.exp(-np.arange(taps) / (taps / 6.0)) * 0.3 + (np.arange(taps) == 20) for _ in range(n)]
    out = torch.empty(int(samples.numel()), device=dev)
    for taps in (1024, 4096):
        plan = hb.ReverbPlan(rirs(taps), max_taps=taps)
        ridx = hb.to_device_i32([b % len(plan) for b in range(B)], dev)
        ms = _timed(lambda: hb.reverb(plan, samples, offs_d, ridx, out, max_len=max(counts)), args.iters)
        flop = 2.0 * sum(counts) * taps
        lines.append(dict(tool="tools/frontend_bench.py", measurement="reverb", taps=taps, workload=workload + ", every row reverberated",
                          samples=int(samples.numel()), gpu_ms_per_launch=round(ms, 4), gflop=round(flop / 1e9, 2),
                          tflop_per_s=round(flop / ms / 1e9, 2), timing=timing))
    clips = [rs.randn(int(16000 * s)) * 500 for s in np.linspace(1.0, 4.0, 8)]
    bank = hb.NoiseBank(clips)
    wav = samples.float()
    cidx = hb.to_device_i32([b % len(bank) for b in range(B)], dev)
    start = hb.to_device_i64([(977 * b) % 16000 for b in range(B)], dev)
    scale = hb.to_device_f32(np.full(B, 0.1, np.float32), dev)
    ms = _timed(lambda: hb.noise_mix(bank, wav, offs_d, cidx, start, scale, max_len=max(counts)), args.iters)
    moved = int(wav.numel()) * 4 * 5                        # y and v read twice, z written once
    lines.append(dict(tool="tools/frontend_bench.py", measurement="noise_mix", workload=workload + " as float32, every row mixed, in place",
                      samples=int(wav.numel()), gpu_ms_per_call=round(ms, 4), launches_per_call=2, bytes_moved=moved,
                      gb_per_s=round(moved / ms / 1e6, 1), timing=timing))
    if args.skip_epoch_loop:
        return lines
    tmp = tempfile.mkdtemp(prefix="frontend_bench_")
    sv = bench.make_solver(c, B, T, os.path.join(tmp, "cfg2"))
    base = dict(n_mels=80, delta_order=0, cmvn="utterance")
    keys = dict(reverb=dict(bank=_bank(rirs(4096)), prob=0.5, max_taps=4096), noise=dict(bank=_bank(clips), prob=0.5, snr_db=[5, 20]))
    fes = {"plain": Frontend(base), "augment": Frontend(dict(base, **keys))}
    n = args.warmup + args.steps

    def window(kind):
        feed = DeviceFeed([items] * n, dev, frontend=fes[kind], train=True)
        with contextlib.redirect_stdout(sys.stderr):
            for i, (xs, ilens, ys) in enumerate(feed):
                if i == args.warmup:
                    sv.flush()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                last = sv.sup_train_one_iteration(xs, ilens, ys, 1.0)
            sv.flush()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(last)
    windows, loss = {k: [] for k in fes}, {}
    np.random.seed(1234)                                  # the feeds' augment seeds
    for _ in range(args.rounds):
        for kind in fes:
            ms, loss[kind] = window(kind)
            windows[kind].append(ms)
    med = {k: statistics.median(w) for k, w in windows.items()}
    for kind in fes:
        lines.append(dict(tool="tools/frontend_bench.py", measurement="epoch_loop_augment", feed=kind,
                          call="Solver.sup_train_one_iteration",
                          workload="%s, batch %d, waveforms U[0.6, 1] x 8 s, training feed.DeviceFeed" % (spec["name"], B),
                          augment="reverb 8 x 4096 taps prob 0.5, noise 8 clips prob 0.5 snr_db [5, 20]" if kind == "augment" else None,
                          rounds=args.rounds, steps_per_window=args.steps, warmup_steps=args.warmup,
                          ms_per_step=round(med[kind], 3), windows_ms=[round(w, 3) for w in windows[kind]],
                          spread=round((max(windows[kind]) - min(windows[kind])) / med[kind], 4),
                          over_plain=round(med[kind] / med["plain"], 4), last_loss=loss[kind], arith=hb.arith_name()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-epoch-loop", action="store_true")
    ap.add_argument("--speed", action="store_true", help="measure speed perturbation instead (resample, epoch_loop_speed)")
    ap.add_argument("--augment", action="store_true",
                    help="measure reverberation and noise instead (reverb, noise_mix, epoch_loop_augment)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_bench.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import hip_backend as hb
    from dataset import synthetic_utterances, synthetic_waveforms
    from feed import DeviceFeed
    from frontend import Frontend
    assert torch.cuda.is_available(), "frontend_bench.py measures on the GPU"
    dev = torch.device("cuda")
    spec = bench.CONFIGS["cfg2"]
    c, B, T = dict(spec["model"]), spec["batch"], spec["frames"]
    data = synthetic_waveforms(B, c["output_dim"], 8.0, seed=1234)
    items = sorted([(v["feature"], v["token_ids"]) for v in data.values()], key=lambda it: -len(it[0]))
    waves = [f for f, _ in items]
    offs = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).tolist()
    samples = torch.from_numpy(np.concatenate(waves)).to(dev)
    threads = bench.usable_cpus()
    lines = []

    if args.speed:
        lines = speed_lines(args, bench, hb, spec, items, samples, offs)
    if args.augment:
        lines = augment_lines(args, bench, hb, spec, items, samples, offs)
    for order in (() if args.speed or args.augment else (0, 2)):
        fe = Frontend(dict(n_mels=80, delta_order=order, cmvn="utterance"))
        for _ in range(5):
            xs, ilens = fe(samples, offs)
        torch.cuda.synchronize()
        hb.LAUNCHES.clear()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            xs, ilens = fe(samples, offs)
        stop.record()
        torch.cuda.synchronize()
        gpu_ms = start.elapsed_time(stop) / args.iters
        cpu_ms = cpu_frontend(waves, order, threads) * 1e3
        frames = sum(ilens)
        lines.append(dict(tool="tools/frontend_bench.py", measurement="front_end", delta_order=order, cmvn="utterance",
                          workload="%d ragged utterances, U[0.6, 1] x 8 s int16 at 16 kHz, 80 bins" % B, frames=frames,
                          samples=int(samples.numel()), upload_bytes_waveform=int(samples.numel()) * 2,
                          upload_bytes_features=B * max(ilens) * fe.output_dim * 4,
                          gpu_ms_per_batch=round(gpu_ms, 4), launches_per_batch={k: v // args.iters for k, v in hb.LAUNCHES.items()},
                          timing="device events around %d calls (host enqueue included), samples resident" % args.iters,
                          cpu_torch_ms_per_batch=round(cpu_ms, 2), cpu_threads=threads, cpu_over_gpu=round(cpu_ms / gpu_ms, 1)))

    if not args.skip_epoch_loop and not args.speed and not args.augment:
        tmp = tempfile.mkdtemp(prefix="frontend_bench_")
        fe = Frontend(dict(n_mels=80, delta_order=0, cmvn="utterance"))
        assert fe.output_dim == c["input_dim"]
        sv = bench.make_solver(c, B, T, os.path.join(tmp, "cfg2"))
        feats = synthetic_utterances(B, c["input_dim"], c["output_dim"], T, seed=1234)
        f_items = sorted([(v["feature"], v["token_ids"]) for v in feats.values()], key=lambda it: -len(it[0]))
        # the same frame counts and labels on either side: features cut to the front end's frame count of each waveform
        f_items = [(np.resize(f, (fe.num_frames(len(w)), c["input_dim"])).astype(np.float32), y)
                   for (f, _), (w, y) in zip(f_items, items)]
        n = args.warmup + args.steps

        def window(kind):
            source = [items if kind == "waveforms" else f_items] * n
            feed = DeviceFeed(source, dev, frontend=fe if kind == "waveforms" else None)
            with contextlib.redirect_stdout(sys.stderr):
                for i, (xs, ilens, ys) in enumerate(feed):
                    if i == args.warmup:
                        sv.flush()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    last = sv.sup_train_one_iteration(xs, ilens, ys, 1.0)
                sv.flush()
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3, float(last)
        windows, loss = {"features": [], "waveforms": []}, {}
        for _ in range(args.rounds):
            for kind in ("features", "waveforms"):
                ms, loss[kind] = window(kind)
                windows[kind].append(ms)
        med = {k: statistics.median(w) for k, w in windows.items()}
        lines.append(dict(tool="tools/frontend_bench.py", measurement="epoch_loop", call="Solver.sup_train_one_iteration",
                          workload="%s, batch %d, 80 x <= %d frames, fed by feed.DeviceFeed" % (spec["name"], B, fe.num_frames(128000)),
                          rounds=args.rounds, steps_per_window=args.steps, warmup_steps=args.warmup,
                          ms_per_step_features=round(med["features"], 3), ms_per_step_waveforms=round(med["waveforms"], 3),
                          waveforms_over_features=round(med["waveforms"] / med["features"], 4),
                          windows_ms_features=[round(w, 3) for w in windows["features"]],
                          windows_ms_waveforms=[round(w, 3) for w in windows["waveforms"]],
                          spread_features=round((max(windows["features"]) - min(windows["features"])) / med["features"], 4),
                          spread_waveforms=round((max(windows["waveforms"]) - min(windows["waveforms"])) / med["waveforms"], 4),
                          last_loss=loss, arith=hb.arith_name()))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in lines:
            line = json.dumps(rec)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()

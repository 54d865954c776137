"""Deterministic mode on the GPU (include/asr_hip.h "Deterministic mode").
1. asr_gemm_det_f32 IS the ordered sum of unsplit slab products the header describes (bit for bit), and an fp32 product.
2. Every ordered reduction: right against float64, the same bits on every call, the same bits beside another stream's work.
3. A whole train step reproduces: loss, every parameter and every Adam state tensor, bit for bit, step after step.
4. The mode is the same model (the golden fixture, the gates of the default path).
5. Nothing of the mode is left behind when it is switched off."""
import os
import pickle

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


DEV = "cuda"
LOSS_GATE = (1e-5, 1e-5)          # rtol, atol of the loss against the golden fixture (test_the_mode_is_the_same_model)
GRAD_GATE = (1e-3, 1e-6)          # rtol, atol of every gradient against the golden fixture (same test)
LOGPROB_GATE = (1e-5, 1e-6)       # rtol, atol of test_label_logprob_kernels (test_loss_total_det)


def _close(got, want, rtol, atol, what=""):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    scale = max(1e-30, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= atol + rtol * scale, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


_BIG = {}


def _same_bits_every_time(call, what):
    """8 calls on the same input give the same bits, and so does a call issued while a second stream runs an unrelated large
    product (workgroups of the two share the chip: another arrival order)."""
    import hip_backend as hb
    first = call().clone()
    for i in range(7):
        assert torch.equal(call(), first), "%s: call %d differs from the first" % (what, i + 2)
    if not _BIG:
        g = torch.Generator().manual_seed(1)
        _BIG.update(a=torch.randn(4096, 4096, generator=g).to(DEV), b=torch.randn(4096, 4096, generator=g).to(DEV),
                    out=torch.empty(4096, 4096, device=DEV), side=torch.cuda.Stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(_BIG["side"]), hb.deterministic(False):
        hb.gemm(_BIG["a"], _BIG["b"], out=_BIG["out"])
    beside = call().clone()
    torch.cuda.synchronize()
    assert torch.equal(beside, first), "%s: differs beside another stream's product" % what
    return first


# ------------------------------------------------------------------------------------------------------------ 1
def _slabs(hb, A, B, ta, tb, S, kper, K):
    out = []
    for s in range(S):
        k0, k1 = s * kper, min(K, (s + 1) * kper)
        As = A[k0:k1] if ta else A[:, k0:k1]
        Bs = B[:, k0:k1] if tb else B[k0:k1]
        with hb.deterministic(False):
            out.append(hb.gemm(As, Bs, trans_a=ta, trans_b=tb, split_k=1))
    return out


@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("split", [None, 2, 3, 7])
def test_gemm_det_is_the_ordered_sum_of_its_slabs(hb, ta, tb, split):
    """C = (((ws[0] + ws[1]) + ...) + ws[S-1]) (+ bias) (+ C) (relu), the header's order: slab s is the unsplit product of K range s - formed here
    by hb.gemm(split_k=1) on the same operand views, added by torch in fp32 in slab order.  The slabs of one call run as the
    batch of one launch; the test first makes sure that batch and the single product take the same kernel (at these sizes the
    64 x 64 tiles either way), so the comparison is of the same arithmetic - bit for bit, whatever ran when."""
    g = torch.Generator().manual_seed(17 + 2 * ta + tb + (split or 0))
    case = 0
    for K in (1, 63, 1000, 2051):
        for M in (1, 17, 80, 130):
            for N in (1, 17, 80, 130):
                info = hb.gemm_det_split(M, N, K, trans_a=ta, trans_b=tb, split=split)
                assert info["rc"] == 0
                S, kper = info["split"], info["k_range"]
                if split is None and S == 1:
                    continue                       # (the rule splits only the long K: every shape at K = 2 051)
                case += 1
                A = torch.randn((K, M) if ta else (M, K), generator=g).to(DEV)
                B = torch.randn((N, K) if tb else (K, N), generator=g).to(DEV)
                bias = torch.randn(N, generator=g).to(DEV) if case & 1 else None
                relu = bool(case & 2)
                prev = torch.randn(M, N, generator=g).to(DEV) if case & 4 else None
                if S > 1:
                    one = hb.gemm_plan(M, N, kper, trans_a=ta, trans_b=tb, lda=A.stride(0), ldb=B.stride(0), split_k=1)
                    many = hb.gemm_plan(M, N, kper, trans_a=ta, trans_b=tb, lda=A.stride(0), ldb=B.stride(0), split_k=1,
                                        batch=K // kper, sA=kper * (A.stride(0) if ta else 1),
                                        sB=kper * (1 if tb else B.stride(0)), sC=M * N)
                    assert one["kernel"] == many["kernel"] and one["tile"] == many["tile"], (one, many)
                want = None
                for slab in _slabs(hb, A, B, ta, tb, S, kper, K):
                    want = slab if want is None else want + slab
                if bias is not None:
                    want = want + bias
                if prev is not None:
                    want = want + prev
                if relu:
                    want = torch.relu(want)
                out = prev.clone() if prev is not None else torch.full((M, N), 7.0, device=DEV)
                hb.gemm_det(A, B, trans_a=ta, trans_b=tb, bias=bias, relu=relu, out=out, accumulate=prev is not None, split=split)
                assert torch.equal(out, want), ("M %d N %d K %d S %d bias %s relu %s acc %s: max diff %.3g"
                                                % (M, N, K, S, bias is not None, relu, prev is not None,
                                                   float((out - want).abs().max())))
    assert case >= (16 if split is None else 64)


@pytest.mark.parametrize("ta,tb,M,N,K,split", [(True, False, 130, 80, 2051, None), (False, True, 80, 130, 2051, 7),
                                               (False, False, 17, 130, 1000, 3), (True, True, 130, 17, 63, 2),
                                               (True, False, 512, 160, 4100, None)])
def test_gemm_det_is_an_fp32_product(hb, ta, tb, M, N, K, split):
    """Against a float64 product of the same operands, under the bound test_gemm_bf16x6_is_fp32_equivalent holds the bf16x6
    products to: within 2x the error of the exact-fp32 unsplit kernel (+ 2e-8), relative to the largest output."""
    g = torch.Generator().manual_seed(M + 3 * N + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    scale = float(ref.abs().max())
    with hb.deterministic(False):
        e32 = float((hb.gemm(A.to(DEV), B.to(DEV), trans_a=ta, trans_b=tb, arith="f32", split_k=1).double().cpu() - ref).abs().max()) / scale
    assert hb.gemm_det_split(M, N, K, trans_a=ta, trans_b=tb, split=split)["split"] > 1
    Ad, Bd = A.to(DEV), B.to(DEV)
    out = _same_bits_every_time(lambda: hb.gemm_det(Ad, Bd, trans_a=ta, trans_b=tb, split=split), "gemm_det")
    e6 = float((out.double().cpu() - ref).abs().max()) / scale
    print("gemm_det %dx%dx%d: error %.3g, fp32 kernel %.3g" % (M, N, K, e6, e32))
    assert e6 <= 2.0 * e32 + 2e-8, "error %.3g vs fp32 kernel %.3g" % (e6, e32)


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("N", [1, 68, 260])
@pytest.mark.parametrize("M", [1, 255, 257, 1025])
def test_colsum_det(hb, M, N):
    """Tolerance of test_gemm_skinny_and_colsum (rtol 1e-5 of the largest sum, atol 1e-4); dense and row-strided (ldx > N, where
    N % 4 == 0 keeps the float4 path only if ldx % 4 == 0 too: both are run), with and without accumulate."""
    g = torch.Generator().manual_seed(M + N)
    for pad in (0, 4, 3):
        buf = torch.randn(M, N + pad, generator=g).to(DEV)
        X = buf[:, :N]
        prev = torch.randn(N, generator=g).to(DEV)
        want = X.double().sum(0)
        with hb.deterministic():
            got = _same_bits_every_time(lambda: hb.colsum(X), "colsum %dx%d ld %d" % (M, N, N + pad))
            acc = _same_bits_every_time(lambda: hb.colsum(X, out=prev.clone(), accumulate=True), "colsum accumulate")
        _close(got, want, 1e-5, 1e-4, "colsum")
        _close(acc, want + prev.double(), 1e-5, 1e-4, "colsum accumulate")


@pytest.mark.parametrize("E", [4, 128])
@pytest.mark.parametrize("V", [5, 33])
@pytest.mark.parametrize("rows", [1, 37, 3000])
def test_embedding_grad_det(hb, rows, V, E):
    """Tolerance of test_embedding_grad_kernel (rtol 1e-5, atol 1e-5); a fifth of the rows carry -1, and with rows >> V every
    id repeats many times."""
    g = torch.Generator().manual_seed(rows + V + E)
    KX = E + 12
    buf = torch.randn(rows, KX, generator=g).to(DEV)
    grad = buf[:, KX - E:]
    tok = torch.randint(0, V, (rows,), generator=g)
    tok[torch.rand(rows, generator=g) < 0.2] = -1
    tok = tok.to(DEV)
    acc = torch.randn(V, E, generator=g).to(DEV)
    want = acc.double()
    fed = tok >= 0
    want.index_add_(0, tok[fed], grad[fed].double())

    def call():
        out = acc.clone()
        assert hb.embedding_grad(tok, grad, out)
        return out
    with hb.deterministic():
        got = _same_bits_every_time(call, "embedding gradient")
    _close(got, want, 1e-5, 1e-5, "embedding gradient")


@pytest.mark.parametrize("C", [8, 260])
@pytest.mark.parametrize("relu_gate,seeded", [(False, False), (True, False), (False, True), (True, True)])
def test_pad_fill_grad_det(hb, C, relu_gate, seeded):
    """B = 3, T = 7, one utterance as long as the batch (no padded frame).  A column is a sum of at most (7 - 3) + (7 - 5) = 6
    products: the fp32 error is below 6 * 2^-24 of the sum of magnitudes - held to rtol 1e-5 of the largest entry + 1e-5, the
    tolerance of the other small sums of this file.  The rows of the packed layout must come out as the default entry's."""
    B, T, lens = 3, 7, [7, 5, 3]
    g = torch.Generator().manual_seed(C + 2 * relu_gate + seeded)
    dout = torch.randn(B, T, C, generator=g).to(DEV)
    relu_of = torch.randn(C, generator=g).to(DEV) if relu_gate else None
    rows = hb.LayerRows(hb.RowLayout(lens, [], DEV), 0)
    mask = hb.SeededMask((B, T, C), 0.3, DEV, seed=99) if seeded else None
    m = mask.tensor().double() if seeded else torch.ones(B, T, C, dtype=torch.float64, device=DEV)
    pad = (torch.arange(T, device=DEV)[None, :] >= torch.tensor(lens, device=DEV)[:, None]).double()[:, :, None]
    want = (dout.double() * m * pad).sum((0, 1))
    if relu_gate:
        want = want * (relu_of > 0).double()
    with hb.deterministic(False):
        drows_default, dfill_default = hb.rows_unpack_bwd(dout, rows, C, mask, True, relu_of=relu_of)
    state = {}

    def call():
        state["drows"], dfill = hb.rows_unpack_bwd(dout, rows, C, mask, True, relu_of=relu_of)
        return dfill
    with hb.deterministic():
        got = _same_bits_every_time(call, "pad-fill gradient")
    assert torch.equal(state["drows"], drows_default)
    _close(got, want, 1e-5, 1e-5, "pad-fill gradient")
    _close(dfill_default, want, 1e-5, 1e-5, "pad-fill gradient (default entry)")


@pytest.mark.parametrize("n", [1, 3, 4, 8197, 2 ** 20 + 3])
def test_sumsq_det(hb, n):
    """Tolerance of test_gather_sumsq_kernel: 1e-5 of the sum.  The word accumulates (the protocol of the update kernel's
    zero_word): a second call adds to the first."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(DEV)
    want = float((x.double() ** 2).sum())
    with hb.deterministic():
        got = _same_bits_every_time(lambda: hb.sumsq(x, torch.zeros(1, device=DEV)), "sumsq")
        twice = hb.sumsq(x, hb.sumsq(x, torch.zeros(1, device=DEV)))
    assert abs(float(got) - want) <= 1e-5 * want
    assert float(twice) == float(got + got)


def test_gather_sumsq_det(hb):
    """The job list of test_gather_sumsq_kernel (more jobs than one launch carries, odd sizes, a source that is not 16-byte
    aligned) plus the sizes of test_sumsq_det; its tolerance."""
    g = torch.Generator().manual_seed(17)
    sizes = [1, 3, 4, 5, 4096, 4097, 12345, 8197, 2 ** 20 + 3, 7] + [33] * 70
    srcs, offs, off = [], [], 0
    for i, n in enumerate(sizes):
        t = torch.randn(n + 1, generator=g).to(DEV)
        srcs.append(t[1:] if i == 6 else t[:n])
        offs.append(off)
        off += (n + 3) // 4 * 4
    flat = torch.full((off,), 7.0, device=DEV)
    with hb.deterministic():
        got = _same_bits_every_time(lambda: (hb.gather_sumsq(srcs, offs, flat, acc := torch.zeros(1, device=DEV)), acc)[1],
                                    "gather + sumsq")
        keep = flat.clone()
        hb.gather_sumsq(srcs[:3], offs[:3], flat, None)
    assert torch.equal(flat, keep)
    want = 0.0
    for s_, o in zip(srcs, offs):
        assert torch.equal(flat[o:o + s_.numel()], s_)
        want += float((s_.double() ** 2).sum())
    assert abs(float(got) - want) <= 1e-5 * want


@pytest.mark.parametrize("L,B,V", [(5, 7, 34), (100, 33, 9)])
def test_loss_total_det(hb, L, B, V):
    """The `total` of the label log-probability kernel; tolerance of test_label_logprob_kernels (rtol 1e-5, atol 1e-6)."""
    import ops
    g = torch.Generator().manual_seed(L + V)
    logits = (torch.randn(L, B, V, generator=g) * 3).to(DEV)
    idx = torch.randint(0, V, (L, B), generator=g).to(DEV)
    dist = torch.rand(V, generator=g)
    dist = (dist / dist.sum()).to(DEV)
    lp = torch.log_softmax(logits.double(), dim=2)
    ref = 0.95 * torch.gather(lp, 2, idx.unsqueeze(2)).squeeze(2) + 0.05 * torch.sum(lp * dist.double(), dim=2)
    scale = -1.0 / (L * B)
    with hb.deterministic():
        got = _same_bits_every_time(lambda: ops.label_logprob(logits, idx, dist, 0.05, with_sum=True, sum_scale=scale)[1].reshape(1),
                                    "loss total")
    _close(got, (ref.sum() * scale).reshape(1), *LOGPROB_GATE, "loss total")


# ------------------------------------------------------------------------------------------------------------ 3
def _solver(root, monkeypatch, t, l, seeds=(11, 31, 12, 32), **over):
    """A Solver with the model / judge shapes t / l and seeded weights (as test_solver_gpu._tiny_solver)."""
    import yaml
    from dataset import synthetic_utterances
    from solver import Solver
    nv = t["output_dim"]
    vocab = {s: i for i, s in enumerate(["<PAD>", "<BOS>", "<EOS>"] + ["s%d" % i for i in range(nv - 5)] + ["<space>", "<NOISE>"])}
    os.makedirs(root, exist_ok=True)
    for name, n, seed in (("train", 12, 1), ("dev", 4, 2)):
        with open(os.path.join(root, name + ".pkl"), "wb") as f:
            pickle.dump(synthetic_utterances(n, t["input_dim"], nv, 24, seed), f)
    with open(os.path.join(root, "vocab_dict.pkl"), "wb") as f:
        pickle.dump(vocab, f)
    with open(os.path.join(root, "non_lang_syms.pkl"), "wb") as f:
        pickle.dump(["<NOISE>", "<PAD>", "<BOS>", "<EOS>"], f)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "semi-supervised-asr_amd", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(logdir=os.path.join(root, "log"), model_dir=root, model_name="m", load_model_path=os.path.join(root, "m"),
               load_judge_path=os.path.join(root, "m"), dataset_root_dir=root, vocab_path=os.path.join(root, "vocab_dict.pkl"),
               non_lang_syms_path=os.path.join(root, "non_lang_syms.pkl"), labeled_set="train", unlabeled_speech_set="train",
               unlabeled_text_set="train", dev_set="dev", test_set="dev", max_dec_timesteps=8, batch_size=4,
               input_dim=t["input_dim"], enc_hidden_dim=t["enc_hidden_dim"], enc_n_layers=t["enc_n_layers"],
               subsample=t["subsample"], dropout_rate=0.0, dec_hidden_dim=t["dec_hidden_dim"], att_dim=t["att_dim"],
               conv_channels=t["conv_channels"], conv_kernel_size=t["conv_kernel_size"], att_odim=t["att_odim"],
               embedding_dim=t["embedding_dim"], ls_weight=t["ls_weight"], dis_embedding_dim=l["embedding_dim"],
               dis_hidden_dim=l["hidden_dim"], dis_dropout_rate=0.0, dis_layers=l["n_layers"], d_learning_rate=2e-4,
               learning_rate=5e-4, weight_decay=1e-6, max_grad_norm=5, unsup_weight=0.5, smooth_embedding=True,
               softmax_scaling=3, min_feature_length=1, add_gaussian=False)
    cfg.update(over)
    monkeypatch.chdir(root)
    solver = Solver(cfg)
    dev = next(solver.model.parameters()).device
    with torch.no_grad():
        wm, wj = synth.e2e_weights(t, seeds[0]), synth.lm_weights(l, seeds[1])
        for k, v in solver.model.state_dict().items():
            v.copy_(torch.from_numpy(wm[k]))
        for k, v in solver.judge.state_dict().items():
            v.copy_(torch.from_numpy(wj[k]))
    for mod, seed in ((solver.model.decoder, seeds[2]), (solver.judge, seeds[3])):
        mod.labeldist = synth.labeldist(nv, seed)
        mod.vlabeldist = torch.from_numpy(np.asarray(mod.labeldist, dtype=np.float32)).to(dev)
    solver.model.decoder._dist_dev = {}
    solver.judge._dist_dev = {}
    solver.proportion = 0.5
    solver.model.train()
    solver.judge.train()
    return solver, dev


def _state(solver, opt):
    out = {"p/" + n: p.detach().clone() for n, p in list(solver.model.named_parameters()) + list(solver.judge.named_parameters())}
    out.update(m=opt.m.clone(), v=opt.v.clone())
    if opt.vmax is not None:
        out["vmax"] = opt.vmax.clone()
    return out


def _run_twice(tmp_path, monkeypatch, t, l, steps, cfg, after_build=None):
    """steps(solver, dev) yields (label, loss, optimiser) after every train step.  Two Solvers built from the same state and
    seeds: the loss and every parameter and Adam state tensor after every step, bit for bit."""
    import hip_backend as hb
    records = []
    for run in range(2):
        solver, dev = _solver(str(tmp_path / ("run%d" % run)), monkeypatch, t, l, deterministic=True, **cfg)
        assert solver.deterministic and not hb.is_deterministic()
        torch.manual_seed(3)
        np.random.seed(4)
        hb.persist_clear_abort(dev)
        hb.LAUNCHES.clear()
        rec = []
        for label, loss, opt in steps(solver, dev):
            solver.flush()
            rec.append((label, float(loss), _state(solver, opt)))
        assert not hb.persist_aborted(dev)
        if after_build is not None:
            after_build(dict(hb.LAUNCHES))
        records.append(rec)
    assert len(records[0]) == len(records[1]) > 0
    for (la, loss_a, sa), (lb, loss_b, sb) in zip(*records):
        assert la == lb and np.isfinite(loss_a)
        assert loss_a == loss_b, "%s: loss %.9g vs %.9g" % (la, loss_a, loss_b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), "%s: %s differs between the two runs (max %.3g)" % (
                la, k, float((sa[k] - sb[k]).abs().max()))
    return records[0]


def _sup_steps(batch, n=5, tf_rate=0.5):
    def steps(solver, dev):
        xs, ilens, ys = batch
        xs_d, ys_d = torch.from_numpy(xs).to(dev), [torch.from_numpy(y).to(dev) for y in ys]
        for i in range(n):
            yield "sup step %d" % i, solver.sup_train_one_iteration(xs_d, ilens, ys_d, tf_rate), solver.gen_opt
    return steps


def test_supervised_steps_reproduce_at_the_tiny_shape(hb, tmp_path, monkeypatch):
    """5 x sup_train_one_iteration on the ragged tiny_e2e batch, dropout 0.3, tf_rate 0.5 (scheduled sampling: the free-running
    decoder and its backward), on the per-step kernels of every sequence operator."""
    batch = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    rec = _run_twice(tmp_path, monkeypatch, synth.TINY, synth.TINY_LM, _sup_steps(batch), dict(dropout_rate=0.3))
    assert len(set(r[1] for r in rec)) == 5, "five different steps"


def test_supervised_steps_reproduce_on_the_persistent_lstm_kernels(hb, tmp_path, monkeypatch):
    """The same at the smallest shape the persistent LSTM kernels serve (H = 128; B = 8, T = 48), asserted on the launch
    counters as hb.require_persistent does: no encoder layer ran on the per-step kernels, forward or backward."""
    t = dict(synth.TINY, input_dim=16, enc_hidden_dim=128)
    batch = synth.ragged_batch(8, 48, 16, 9, 21)

    def paths(launches):
        assert launches.get("lstm_fwd_persist", 0) >= 10 and launches.get("lstm_bwd_persist", 0) >= 10, launches
        assert "lstm_fwd_step" not in launches and "lstm_bwd_step" not in launches, launches
        assert launches.get("dec_bwd_det", 0) == 5 and "dec_bwd_persist" not in launches, launches
    if not hb.USE_PERSIST:
        pytest.fail("the persistent kernels are switched off in this process")
    _run_twice(tmp_path, monkeypatch, t, synth.TINY_LM, _sup_steps(batch), dict(dropout_rate=0.3), after_build=paths)


def test_judge_and_generator_steps_reproduce(hb, tmp_path, monkeypatch):
    """One judge_train_one_iteration and one gen_train_one_iteration (smooth-embedding feedback, both model passes) at the
    tiny_ssl shape."""
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    uxs, uilens, _ = synth.batch(8, 9, [12, 10, 7], [2, 2, 2], 41)

    def steps(solver, dev):
        ys_d = [torch.from_numpy(y).to(dev) for y in ys]
        yield "judge", solver.judge_train_one_iteration(ys_d)["loss"], solver.dis_opt
        meta = solver.gen_train_one_iteration(torch.from_numpy(xs).to(dev), ilens, ys_d, torch.from_numpy(uxs).to(dev), uilens)
        yield "generator", meta["loss"], solver.gen_opt
    _run_twice(tmp_path, monkeypatch, synth.TINY, synth.TINY_LM, steps, dict(dropout_rate=0.3, dis_dropout_rate=0.3))


# ------------------------------------------------------------------------------------------------------------ 4, 5
def _tiny_net(golden_dir):
    import model as M
    g = dict(np.load(os.path.join(golden_dir, "tiny_e2e.npz"), allow_pickle=False))
    net = M.E2E(labeldist=g["labeldist"], **synth.TINY).to(DEV)
    missing = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.e2e_weights(synth.TINY, 11).items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    net.train()
    xs, ilens, ys = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13)
    return g, net, torch.from_numpy(xs).to(DEV), ilens, [torch.from_numpy(y).to(DEV) for y in ys]


def _tiny_step(net, xs, ilens, ys):
    np.random.seed(5)
    logits, lp, pred, ws = net(xs, ilens, ys, tf_rate=1.0)
    loss = -lp.mean()
    net.zero_grad()
    loss.backward()
    return logits, lp, ws, loss


def test_the_mode_is_the_same_model(hb, golden_dir):
    """Loss and gradients of the tiny_e2e fixture in deterministic mode, under the gates of test_tiny_e2e_teacher_forced."""
    g, net, xs, ilens, ys = _tiny_net(golden_dir)
    with hb.deterministic():
        logits, lp, ws, loss = _tiny_step(net, xs, ilens, ys)
    _close(logits, torch.from_numpy(g["tf_logits"]), 1e-3, 1e-5, "logits")
    _close(lp, torch.from_numpy(g["tf_lp"]), 1e-3, 1e-5, "lp")
    _close(ws, torch.from_numpy(g["tf_ws"]), 1e-3, 1e-5, "ws")
    _close(loss, torch.from_numpy(g["tf_loss"]), *LOSS_GATE, "loss")
    for n, p in net.named_parameters():
        _close(p.grad, torch.from_numpy(g["grad/" + n]), *GRAD_GATE, "grad " + n)


def test_nothing_leaks_out_of_the_mode(hb, golden_dir):
    """Two default steps around a deterministic one take the same paths (hb.LAUNCHES), and the deterministic one took its own."""
    _, net, xs, ilens, ys = _tiny_net(golden_dir)
    assert not hb.is_deterministic()
    paths = []
    for det in (False, True, False):
        hb.LAUNCHES.clear()
        with hb.deterministic(det):
            _tiny_step(net, xs, ilens, ys)
        paths.append(dict(hb.LAUNCHES))
        assert not hb.is_deterministic()
    assert paths[0] == paths[2], paths
    assert "dec_bwd_det" not in paths[0] and paths[1].get("dec_bwd_det") == 1, paths
    assert sum(v for k, v in paths[0].items() if k.startswith("dec_bwd")) == 1

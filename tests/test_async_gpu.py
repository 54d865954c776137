"""No result may depend on how far the host runs ahead of the GPU (tests/async_cases.py has the harness and the rules).

Every case enqueues a delay kernel, then does - without waiting - what the next step of a real program does while this one
is still queued: the call under test with its own uploads, 16 further uploads of the same sizes with other values, the same
operator on other inputs of the same shapes, the first call's inputs dropped and their memory refilled with NaN.  It then
asserts that the delay was STILL running (a case that cannot show this fails), lets the GPU catch up and compares every
output with the same host phase run synchronously: bit for bit.  Everything that reaches split-K atomics runs under
hb.deterministic(); the sequence kernels and the front end promise the same bits in every run.

Each case prints `async-invariance <case> host <ms> stall <ms> proved 1 words <compared>/<differing>` (pytest -s;
profiles/async_invariance.txt holds one run).

No case can fault: every length and offset uploaded, the scribbled ones included, is valid for the shapes it could meet."""
import time

import numpy as np
import pytest
import torch

import async_cases as A
import batch_cases as B
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


@pytest.fixture
def in_stream(hb):
    """The small batches of this module would take the in-stream copies anyway: said explicitly, and put back."""
    saved = hb.UPLOAD_SIDE_STREAM[0]
    hb.UPLOAD_SIDE_STREAM[0] = False
    try:
        yield
    finally:
        hb.UPLOAD_SIDE_STREAM[0] = saved


def _lens_alternatives(lens, T):
    """Other VALID frame counts for the same rows: reversed, all 1, all T, each one shorter (>= 0)."""
    lens = [int(n) for n in lens]
    return [lens[::-1], [min(1, T)] * len(lens), [T] * len(lens), [max(n - 1, 0) for n in lens]]


def test_a_stall_lasts_what_was_asked(hb):
    """The harness itself: a 50 ms and a 200 ms stall last that long by the device's own events (within 20 %) - a stall
    that ends early lets a case fail for nothing, one that runs long wastes the suite's time."""
    for ms in (50.0, 200.0):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        st = A.stalled(None, ms)
        b.record()
        assert st.proved()
        b.synchronize()
        took = a.elapsed_time(b)
        print("async-invariance stall asked %.0f ms lasted %.1f ms" % (ms, took))
        assert 0.8 * ms <= took <= 1.2 * ms and not st.proved()


# ------------------------------------------------------------------------------------------------- 1, 2: the upload ring
UPLOADS = [("i32", 4), ("i64", 5), ("f32", 4)]
N_UPLOADS = 3 * 8 + 1


def _upload_values(kind, n):
    return [(np.arange(n) + 1 + 100 * i).astype(np.float32 if kind == "f32" else np.int64) for i in range(N_UPLOADS)]


def _ring_case(hb, kind, n, side):
    up = dict(i32=hb.to_device_i32, i64=hb.to_device_i64, f32=hb.to_device_f32)[kind]
    values = _upload_values(kind, n)
    saved = hb.UPLOAD_SIDE_STREAM[0]
    hb.UPLOAD_SIDE_STREAM[0] = side
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base = [up(v if kind == "f32" else v.tolist(), DEV) for v in values]
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        del base
        st = A.stalled(None, A.stall_ms(host_ms))
        got = [up(v if kind == "f32" else v.tolist(), DEV) for v in values]
        proved = st.proved()
        torch.cuda.synchronize()
    finally:
        hb.UPLOAD_SIDE_STREAM[0] = saved
    as_sent = dict(i32=np.int32, i64=np.int64, f32=np.float32)[kind]
    bad = sum(int((A.words(g) != A.words(v.astype(as_sent))).sum()) for g, v in zip(got, values))
    print("async-invariance upload-ring %s[%d] %s host %.2f stall %.0f proved %d words %d/%d"
          % (kind, n, "side-stream" if side else "in-stream", host_ms, st.ms, proved, sum(A.words(g).size for g in got), bad))
    assert proved, "the stall had ended before the %d uploads were enqueued: nothing is proven" % N_UPLOADS
    assert bad == 0, "%d of %d uploaded values changed behind a stalled GPU" % (bad, n * N_UPLOADS)


@pytest.mark.parametrize("kind,n", UPLOADS)
def test_upload_ring_in_stream(hb, kind, n):
    """3 x 8 + 1 uploads of one size behind a stall, the copies on the stalled compute stream: each tensor holds its own
    values once the stall has ended - no pinned source was rewritten before its copy ran."""
    _ring_case(hb, kind, n, side=False)


@pytest.mark.parametrize("kind,n", UPLOADS)
def test_upload_ring_side_stream(hb, kind, n):
    _ring_case(hb, kind, n, side=True)


def test_side_stream_upload_reaches_its_consumer_and_is_not_handed_out_early(hb):
    """Side-stream mode: the copy runs at once on the upload stream, its consumer waits behind the stall on the compute
    stream.  25 rounds of: upload lengths, ops.ctc_greedy with them, drop the lengths, allocate on the compute stream.  The
    next round's upload allocates on the upload stream: without record_stream(main) it would get the block the queued
    consumer has yet to read.  Every round's result equals its synchronous run."""
    import ops
    utts, _ = B.align_utts()
    rows = utts[:4]
    c = B.frames_batch(rows)
    T = c["T"]
    alts = [c["lens"]] + _lens_alternatives(c["lens"], T) + [[min(3 + i, T), 1, min(2 * i, T), T] for i in range(1, 8)]
    logits = torch.nan_to_num(torch.from_numpy(c["buf"]), nan=0.0).to(DEV)

    def rounds():
        outs, junk = [], []
        for i in range(N_UPLOADS):
            lens = hb.to_device_i32(alts[i % len(alts)], DEV)
            outs.append(ops.ctc_greedy(logits, lens))
            del lens
            junk.append(torch.full((4,), 1, dtype=torch.int32, device=DEV))
        return outs, junk

    saved = hb.UPLOAD_SIDE_STREAM[0]
    hb.UPLOAD_SIDE_STREAM[0] = True
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base, junk = rounds()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        base = [[A.words(t).copy() for t in o] for o in base]
        del junk
        st = A.stalled(None, A.stall_ms(host_ms))
        got, junk = rounds()
        proved = st.proved()
        torch.cuda.synchronize()
    finally:
        hb.UPLOAD_SIDE_STREAM[0] = saved
    n = bad = 0
    for g, b in zip(got, base):
        for x, y in zip(g, b):
            x = A.words(x)
            n, bad = n + x.size, bad + int((x != y).sum())
    print("async-invariance upload-consumer side-stream host %.2f stall %.0f proved %d words %d/%d" % (host_ms, st.ms, proved, n, bad))
    assert proved, "the stall had ended before the rounds were enqueued: nothing is proven"
    assert len(set(b[1].tobytes() for b in base)) > 4, "the rounds do not tell their lengths apart"
    assert bad == 0


# ------------------------------------------------------------------------------------------------- 3: sequence operators
def _other(rows):
    """(c): the same utterances in the reverse order - the same B, T, V and packed sizes, other lengths on every row."""
    return list(rows)[::-1]


def _run(hb, name, call, rows, lens_T, extra_scribbles=()):
    lens, T = lens_T
    scribbles = [("i32", _lens_alternatives(lens, T))] + list(extra_scribbles)
    with hb.deterministic(True):
        A.run_case(name, lambda tr: call(tr, rows), lambda tr: call(tr, _other(rows)), scribbles, hb=hb, device=DEV)


@pytest.mark.parametrize("zero_infinity", [True, False])
def test_ctc_loss(hb, in_stream, zero_infinity):
    import ops
    utts, _ = B.ctc_utts()

    def call(tr, rows):
        c = B.frames_batch(rows)
        buf = tr.dev(c["buf"]).requires_grad_()
        nll = ops.ctc_loss(buf[:, :, :c["V"]], hb.to_device_i32(c["lens"], DEV), tr.dev(c["labels"]), c["label_lens"],
                           zero_infinity=zero_infinity)
        nll.backward(tr.dev(c["g"]))
        return dict(nll=nll.detach(), dlogits=buf.grad)
    c = B.frames_batch(utts)
    _run(hb, "ctc_loss zero_infinity=%d" % zero_infinity, call, utts, (c["lens"], c["T"]))


def test_rnnt_joint_and_loss(hb, in_stream):
    import ops
    utts, _ = B.rnnt_utts()

    def call(tr, rows):
        c, j = B.rnnt_batch(rows), B.joint_batch(rows)
        pe, pp = tr.dev(j["pe"]).requires_grad_(), tr.dev(j["pp"]).requires_grad_()
        z = ops.rnnt_joint(pe, pp, hb.to_device_i32(j["lens"], DEV), j["label_lens"])
        z.backward(torch.nan_to_num(tr.dev(j["dz"]), nan=0.0))
        buf = tr.dev(c["buf"]).requires_grad_()
        labels = tr.dev(c["labels"])
        nll = ops.rnnt_loss(buf[..., :c["V"]], hb.to_device_i32(c["lens"], DEV), labels, c["label_lens"])
        nll.backward(tr.dev(c["g"]))
        al = ops.rnnt_align(buf.detach()[..., :c["V"]], hb.to_device_i32(c["lens"], DEV), labels, c["label_lens"])
        out = dict(z=z.detach(), dpe=pe.grad, dpp=pp.grad, nll=nll.detach(), dlogits=buf.grad)
        out.update({"align_" + k: getattr(al, k) for k in ("score", "emit_frame", "token_logp", "frame_labels", "blank_logp", "offsets")})
        return out
    c = B.rnnt_batch(utts)
    _run(hb, "rnnt_joint+loss+align", call, utts, (c["lens"], c["T"]))


def test_ctc_align_and_greedy(hb, in_stream):
    import ops
    utts, _ = B.align_utts()

    def call(tr, rows):
        c = B.frames_batch(rows)
        logits = tr.dev(c["buf"])[:, :, :c["V"]]
        res = ops.ctc_align(logits, hb.to_device_i32(c["lens"], DEV), tr.dev(c["labels"]), c["label_lens"])
        ids, n, frame_tok = ops.ctc_greedy(logits, hb.to_device_i32(c["lens"], DEV))
        return dict(path=res.path, score=res.score, first=res.first, last=res.last, token_logp=res.token_logp,
                    offsets=res.offsets, ids=ids, n=n, frame_tok=frame_tok)
    c = B.frames_batch(utts)
    offs = [c["offsets"].tolist(), [0] * len(c["offsets"])]
    _run(hb, "ctc_align+greedy", call, utts, (c["lens"], c["T"]), [("i64", offs)])


@pytest.mark.parametrize("mode", ["plain", "ngram", "word_lm", "context"])
def test_ctc_beam(hb, in_stream, mode):
    import ops
    utts, _, fixtures = B.beam_utts("a")
    K, names = B.BEAM["a"]["K"], B.MODE_OUTPUTS[mode]

    kws = {id(rows[0]): B.beam_kwargs(mode, fixtures, rows, "base") for rows in (utts, _other(utts))}    # (their tables go up here)

    def call(tr, rows):
        c = B.frames_batch(rows)
        res = ops.ctc_beam(tr.dev(c["buf"])[:, :, :c["V"]], hb.to_device_i32(c["lens"], DEV), K, **kws[id(rows[0])])
        return dict(zip(names, res))
    c = B.frames_batch(utts)
    _run(hb, "ctc_beam %s" % mode, call, utts, (c["lens"], c["T"]))


def test_mwer_loss(hb, in_stream):
    import ops
    utts, _ = B.mwer_utts()

    def call(tr, rows):
        c = B.mwer_batch(rows)
        buf = tr.dev(c["buf"]).requires_grad_()
        loss, parts = ops.mwer_loss(buf[:, :, :c["V"]], tr.dev(c["tokens"]), tr.dev(c["npos"]), tr.dev(c["err"]),
                                    B.MWER_SCALE, n_utts=c["B"])
        loss.backward()
        out = dict(loss=loss.detach().reshape(1), dlogits=buf.grad)
        out.update({k: v for k, v in parts.items() if torch.is_tensor(v)})
        return out
    with hb.deterministic(True):
        A.run_case("mwer_loss", lambda tr: call(tr, utts), lambda tr: call(tr, _other(utts)),
                   [("i32", [[1] * 12, [2] * 12])], hb=hb, device=DEV)


@pytest.mark.parametrize("word_level", [False, True], ids=["edit_distance", "word_edit_distance"])
def test_edit_distance(hb, in_stream, word_level):
    pairs, _ = B.edit_pairs(hb.ED_MAX_COLS)

    def call(tr, rows):
        c = B.pairs_batch(rows)
        hyp, ref, ref_len, hyp_len = (tr.dev(c[k]) for k in ("hyp", "ref", "ref_len", "hyp_len"))
        if word_level:
            res = hb.word_edit_distance(hyp, ref, ref_len, B.ED_SPACE, hyp_len=hyp_len)
        else:
            res = hb.edit_distance(hyp, ref, ref_len, hyp_len=hyp_len)
        return dict(zip(("dist", "hyp_n", "ref_n"), res))
    with hb.deterministic(True):
        A.run_case("word_edit_distance" if word_level else "edit_distance", lambda tr: call(tr, pairs),
                   lambda tr: call(tr, _other(pairs)), [("i32", [[0] * 8, [1] * 8])], hb=hb, device=DEV)


def test_ctc_segment(hb, in_stream):
    import ctc_segment_cases as C
    import ops
    cases = [C.case((34, "small", 1.0, f)) for f in (1, 0)]

    def call(tr, c):
        V, recs = c["V"], c["recs"]
        buf = np.full((len(recs), c["z"].shape[1], V + 3), np.nan, dtype=np.float32)
        for i, (t, _) in enumerate(recs):
            buf[i, :t, :V] = c["z"][i, :t]
        ys = np.array([v for _, us in recs for u in us for v in u], dtype=np.int64)
        res = ops.ctc_segment(tr.dev(buf)[:, :, :V], hb.to_device_i32([t for t, _ in recs], DEV), tr.dev(ys),
                              [[len(u) for u in us] for _, us in recs], free_ends=bool(c["free_ends"]), window=c["window"])
        names = ("path", "score", "first", "last", "token_logp", "utt_logp", "utt_conf", "offsets", "utt_offsets", "rec_utts")
        return {k: getattr(res, k) for k in names if torch.is_tensor(getattr(res, k, None))}
    lens, T = [t for t, _ in cases[0]["recs"]], cases[0]["z"].shape[1]
    with hb.deterministic(True):
        A.run_case("ctc_segment", lambda tr: call(tr, cases[0]), lambda tr: call(tr, cases[1]),
                   [("i32", _lens_alternatives(lens, T))], hb=hb, device=DEV)


def test_rnnt_beam(hb, in_stream):
    """The transducer beam search (TransducerHead.beam -> ops.rnnt_beam) at the first grid case of tests/rnnt_beam_ref.py."""
    import rnnt_beam_ref as BR
    import test_rnnt_beam_gpu as TRB
    p, utts = BR.grid_utterances(*BR.GRID[0])
    head = TRB._head(p)
    K, L = 4, 6

    def call(tr, rows):
        T = max(max(u.shape[0] for u in rows), 1) + 1
        x = np.full((len(rows), T, rows[0].shape[1]), np.nan, np.float32)
        for b, u in enumerate(rows):
            x[b, :u.shape[0]] = u
        with torch.no_grad():
            out = head.beam(tr.dev(x), hb.to_device_i32([u.shape[0] for u in rows], DEV), K, L)
        return {"out%d" % i: t for i, t in enumerate(out) if torch.is_tensor(t)}
    lens = [u.shape[0] for u in utts]
    _run(hb, "rnnt_beam", call, list(utts), (lens, max(lens) + 1))


def test_ctc_prefix_state(hb, in_stream):
    """hb.CtcPrefixState: the constructor's init and three chained score / advance steps over synthetic backpointers and
    tokens (the geometry of test_beam_ctc_gpu._kernel_case: V = 34, T' = 60, K = 4, four ragged utterances); lse and the
    prefix state are compared on the frames of every utterance - nothing writes the ones behind T_b."""
    V, Tp, K, EOS, steps = 34, 60, 4, 2, 3
    lens = [Tp, (2 * Tp) // 3, 1, Tp - 1]
    nb = len(lens)

    def call(tr, seed):
        rs = np.random.RandomState(seed)
        buf = np.full((nb, Tp, V + 3), np.nan, dtype=np.float32)
        for b, n in enumerate(lens):
            buf[b, :n, :V] = rs.randn(n, V) * 3.0
        s = hb.BeamSearch(nb, K, V, 5, EOS, DEV)
        cps = hb.CtcPrefixState(s, tr.dev(buf)[:, :, :V], hb.to_device_i32(lens, DEV), 0, lens)
        def valid(t, shape):                                 # (frames behind T_b are never written: undefined memory)
            t = t.reshape(shape)
            return torch.cat([t[b, ..., :n, :].reshape(-1) for b, n in enumerate(lens)])
        out = dict(lse=valid(cps.lse.unsqueeze(-1), (nb, Tp, 1)), init=valid(cps.state[cps.cur], (nb, K, Tp, 2)))
        for t in range(steps):
            cps.score()
            out["psi%d" % t] = cps.psi.clone()
            s.bp_hist[t].copy_(tr.dev(rs.randint(0, K, size=(nb, K)).astype(np.int32)).view_as(s.bp_hist[t]))
            s.tok_hist[t].copy_(tr.dev(rs.randint(3, V, size=(nb, K)).astype(np.int32)).view_as(s.tok_hist[t]))
            cps.advance(t)
            out["state%d" % t], out["last%d" % t] = valid(cps.state[cps.cur], (nb, K, Tp, 2)), cps.last[cps.cur].clone()
        out["psi_prev"] = cps.psi_prev
        return out
    with hb.deterministic(True):
        A.run_case("ctc_prefix_state init+3x(score,advance)", lambda tr: call(tr, 1), lambda tr: call(tr, 2),
                   [("i32", _lens_alternatives(lens, Tp))], hb=hb, device=DEV)


def test_beam_search_select_reorder_backtrack(hb, in_stream):
    """hb.BeamSearch through Decoder.recognize_beams: 6 steps of select and reorder, then the backtrack (fewer steps than
    the search's first look at its all-done word, ops.BEAM_POLL_STEPS: nothing in it waits for the GPU), K = 4, B = 3."""
    import ops
    import test_beam_gpu as TB
    L, K, lens = 6, 4, [22, 15, 8]
    assert L < 2 * ops.BEAM_POLL_STEPS
    net = TB._decoder_net(320, 30, 128, 35)
    encs = {}
    for seed in (11, 12):
        rs = np.random.RandomState(seed)
        enc = rs.randn(len(lens), max(lens), 128).astype(np.float32)
        for b, n in enumerate(lens):
            enc[b, n:] = 0.1
        encs[seed] = enc

    def call(tr, seed):
        with torch.no_grad():
            toks, scores = net.decoder.recognize_beams(tr.dev(encs[seed]), lens, L, K, nbest=True)
        return dict(tokens=toks, scores=scores)
    with hb.deterministic(True):
        A.run_case("beam_search select+reorder+backtrack", lambda tr: call(tr, 11), lambda tr: call(tr, 12),
                   [("i32", _lens_alternatives(lens, max(lens)))], hb=hb, device=DEV)


# ------------------------------------------------------------------------------------------------- 6: the decoder
@pytest.mark.parametrize("name", ["C10-T60-K1", "smooth-V36-C10-T60-K100"], ids=["teacher-forced", "free-running"])
def test_decoder_sequence(hb, in_stream, name):
    """ops.decoder_sequence forward + backward on the persistent kernels at the smallest shapes of test_decoder_shapes_gpu
    (B = 5, width 512, T' = 60): teacher-forced, and free-running with the smooth feedback; two batches behind one stall."""
    import ops
    import test_decoder_shapes_gpu as TDS
    case = [c.values[0] for c in TDS.TEACHER_CASES + TDS.FREE_CASES if c.values[0]["name"] == name]
    assert len(case) == 1
    xs = {seed: TDS._inputs(dict(case[0], seed=seed)) for seed in (0, 1)}
    case = case[0]

    def call(tr, seed):
        x = xs[seed]
        par = {k: tr.dev(x[k].numpy()).requires_grad_(True) for k in TDS.NAMES}
        opts = dict(L=case["L"], tokens=None if x["tokens"] is None else tr.dev(x["tokens"].numpy()), tf_flags=None,
                    smooth=case["kind"] == "smooth", smooth_scaling=3.0, sample=False, scaling=2.0,
                    xmask=None if x["xmask"] is None else tr.dev(x["xmask"].numpy()), bos=1)
        logits, ws, pred = ops.decoder_sequence(par["P"], par["Q"], par["emb_w"], par["w_ih"], par["w_hh"], par["b_ih"],
                                                par["b_hh"], par["wdec"], par["convw"], par["watt"], par["gvec"], par["bo"],
                                                par["w_out"], par["b_out"], tr.dev(x["w0"].numpy()), opts)
        ((logits * tr.dev(x["dlog"].numpy())).sum() + (ws * tr.dev(x["dws"].numpy())).sum()).backward()
        out = dict(logits=logits.detach(), ws=ws.detach(), pred=pred)
        out.update({"d" + k: par[k].grad for k in TDS.NAMES})
        return out
    before = dict(hb.LAUNCHES)
    with hb.deterministic(True):
        A.run_case("decoder_sequence " + name, lambda tr: call(tr, 0), lambda tr: call(tr, 1), hb=hb, device=DEV)
    assert not hb.persist_aborted(torch.device(DEV))
    assert hb.LAUNCHES[case["fwd"]] - before.get(case["fwd"], 0) == 4, "the forward did not run on the persistent kernel"


# ------------------------------------------------------------------------------------------------- 4: the front end
def test_front_end_two_calls_with_different_draws(hb, in_stream):
    """Frontend.__call__ from waveforms with speed perturbation, reverberation, noise, SpecAugment masks and ragged
    lengths: up to eight uploads per call; two calls with different draws behind one stall, each equal to its own
    synchronous run."""
    import test_augment_gpu as TAU
    from frontend import Frontend
    fe = Frontend(dict(TAU.FE_CFG, delta_order=1, speed_perturb=TAU.SPEEDS, **TAU._augment_cfg()))
    items = TAU._items(5, seed=8, dtype=np.int16)
    wave = np.concatenate([f for f, _ in items])
    offs = np.concatenate([[0], np.cumsum([len(f) for f, _ in items])]).tolist()
    draws = {0: ([0, 2, 1, 0, 2], [(0, 1, 8000, 12.0), (-1, 0, 1499, 5.0), (2, -1, 0, 9.0), (-1, -1, 3, 20.0), (1, 2, 0, 7.5)]),
             1: ([2, 1, 0, 1, 0], [(1, 0, 100, 6.0), (2, 2, 0, 15.0), (-1, 1, 4000, 10.0), (0, -1, 0, 8.0), (-1, 0, 700, 18.0)])}

    def call(tr, which):
        fidx, aug = draws[which]
        counts = [fe.perturbed_samples(len(f), i) for (f, _), i in zip(items, fidx)]
        masks = np.stack([np.asarray(fe.draw_masks(77 + which, 3, r, fe.num_frames(n)), dtype=np.int32).reshape(fe.n_masks, 2)
                          for r, n in enumerate(counts)])
        xs, ilens = fe(tr.dev(wave), offs, masks=masks, factor_index=fidx, augment=aug)
        return dict(xs=xs, ilens=torch.tensor(ilens, dtype=torch.int32))
    B5 = len(items)
    scribbles = [("i32", [[0, 1, 2, 1, 0], [1] * B5, [2, 2, 1, 0, 0]]), ("i64", [[0] * (B5 + 1), offs]),
                 ("i64", [[0] * B5, [1, 2, 3, 4, 5]]), ("f32", [np.full(B5, 0.25, np.float32), np.full(B5, 0.5, np.float32)]),
                 ("i32", [np.zeros((B5, fe.n_masks, 2), np.int32)])]
    with hb.deterministic(True):
        A.run_case("frontend speed+reverb+noise+specaug", lambda tr: call(tr, 0), lambda tr: call(tr, 1), scribbles, hb=hb, device=DEV)


# ------------------------------------------------------------------------------------------------- 5: the LSTM layer
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("persistent", [False, True], ids=["per-step H=16", "persistent H=128"])
def test_lstm_layer_longer_then_shorter_batch(hb, in_stream, persistent, packed):
    """ops.lstm_layer forward + backward, both directions; two different batches back to back behind ONE stall, the second
    shorter than the first: the pooled workspace, the scratch and (packed) the row-base uploads of the first are taken again
    while its kernels are still queued."""
    import test_poison_gpu as TPG
    if persistent:
        Bn, I, H, lens_long = 8, 16, 128, [48, 48, 45, 40, 33, 20, 9, 1]
        lens = [min(n, 36) for n in lens_long]
        if not hb.USE_PERSIST:
            pytest.fail("the persistent kernels are switched off in this process")
    else:
        Bn, I, H, lens_long, lens = 3, 8, 16, [9, 7, 4], [7, 5, 4]
    big = TPG._lstm_inputs(2, Bn, max(lens_long), I, H, lens_long, 11)
    small = TPG._lstm_inputs(2, Bn, max(lens), I, H, lens, 12)

    import ops
    prm = {id(c): [p.to(DEV) for p in c["prm"]] for c in (big, small)}

    def call(tr, c, ln):
        """test_poison_gpu._lstm_run with every host array staged (nothing waits for the stalled stream)."""
        gp = [p.detach().requires_grad_(True) for p in prm[id(c)]]
        x = tr.dev(c["x"].numpy())
        if packed:
            layout = hb.RowLayout(ln, [1], DEV)
            rows = hb.LayerRows(layout, 0)
            xin = hb.rows_pack(x, rows).requires_grad_(True)
            dyp = np.full((rows.R, c["dy"].shape[2]), 7.0, dtype=np.float32)     # noise on the padding rows
            for b_, n_ in enumerate(ln):
                r0 = int(layout.base[0][b_])
                dyp[r0:r0 + n_] = c["dy"][b_, :n_].numpy()
            dy = tr.dev(dyp)
            run = lambda: ops.lstm_layer(xin, None, gp, 2, rows=rows)
        else:
            xin = x.requires_grad_(True)
            lens_dev = hb.to_device_i32(ln, DEV)
            dy = tr.dev(c["dy"].transpose(0, 1).contiguous().numpy())
            run = lambda: ops.lstm_layer(xin.transpose(0, 1), lens_dev, gp, 2)
        if persistent:
            with hb.require_persistent():
                y = run()
                y.backward(dy)
        else:
            y = run()
            y.backward(dy)
        out = dict(y=y.detach(), dx=xin.grad)
        out.update({"dprm%d" % i: p.grad for i, p in enumerate(gp)})
        return out
    name = "lstm %s %s" % ("persistent H=128" if persistent else "per-step H=16", "packed" if packed else "padded")
    with hb.deterministic(True):
        A.run_case(name, lambda tr: call(tr, big, lens_long), lambda tr: call(tr, small, lens),
                   [("i32", _lens_alternatives(lens_long, max(lens_long)))], hb=hb, device=DEV)
    assert not hb.persist_aborted(torch.device(DEV))


# ------------------------------------------------------------------------------------------------- 7: two steps in flight
@pytest.mark.parametrize("ctc_weight", [0.0, 0.3])
def test_two_train_steps_in_flight(hb, in_stream, ctc_weight):
    """The tiny E2E model, deterministic mode, ops.step_arena: forward + backward + optimiser step for batch 1 and then for
    batch 2 with no synchronise, behind a stall; every parameter afterwards has the bits of the same two steps with a
    torch.cuda.synchronize() after every call."""
    import model as M
    import ops
    from parallel import FlatAdam
    torch.manual_seed(17)
    proto = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), ctc_weight=ctc_weight, **synth.TINY)
    state = {k: v.clone() for k, v in proto.state_dict().items()}
    state.update({k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()})
    batches = [synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13),
               synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], synth.TINY_ILENS[::-1], synth.TINY_YLENS[::-1], 14)]
    dev = torch.device(DEV, torch.cuda.current_device())

    def one_step(net, opt, i, xs, ilens, ys):
        np.random.seed(5 + i)
        with hb.deterministic(True), ops.step_arena(dev):
            _, lp, _, _ = net(xs, ilens, ys, tf_rate=1.0)
            loss = -lp.mean()
            opt.zero_grad()
            loss.backward()
            opt.step()

    def steps(sync_each):
        net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), ctc_weight=ctc_weight, **synth.TINY).to(dev)
        net.load_state_dict(state)
        net.train()
        opt = FlatAdam(net, lr=5e-4, weight_decay=1e-6, amsgrad=True, max_grad_norm=5.0)
        data = [(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys]) for xs, ilens, ys in batches]
        one_step(net, opt, 0, *data[0])                     # (one step first: a fresh model uploads its constants once)
        torch.cuda.synchronize()
        st = None if sync_each else A.stalled(None, steps.ms)
        t0 = time.perf_counter()
        for i, (xs, ilens, ys) in enumerate(data):
            one_step(net, opt, i, xs, ilens, ys)
            if sync_each:
                torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        proved = None if st is None else st.proved()
        torch.cuda.synchronize()
        return {n: p.detach().clone() for n, p in net.named_parameters()}, host_ms, proved

    steps.ms = A.MIN_MS
    steps(True)                                             # (warms the pools: the timed run allocates nothing new)
    want, host_ms, _ = steps(True)
    steps.ms = A.stall_ms(host_ms)
    got, _, proved = steps(False)
    n, bad = A.differing(got, want)
    print("async-invariance two-steps ctc_weight=%.1f host %.2f stall %.0f proved %d words %d/%d" % (ctc_weight, host_ms, steps.ms, proved, n, bad))
    assert proved, "the stall had ended before both steps were enqueued: nothing is proven"
    assert bad == 0, "%d of %d parameter words differ when two steps are in flight" % (bad, n)
    assert any(not torch.equal(got[k].cpu(), state[k]) for k in got), "the steps changed nothing"


def test_two_ssl_generator_steps_in_flight(hb, in_stream, tmp_path, monkeypatch):
    """Solver.gen_train_one_iteration (two model passes and the judge; deterministic mode, the step arena) for batch 1 and
    then batch 2 with no synchronise, behind a stall (pipeline_steps = 6: nothing is read back in between); the generator's
    parameters and both reported records equal the same two steps with a synchronise after each."""
    import test_deterministic_gpu as TD
    b1 = synth.batch(8, 9, synth.TINY_ILENS, synth.TINY_YLENS, 13) + synth.batch(8, 9, [12, 10, 7], [2, 2, 2], 41)[:2]
    b2 = synth.batch(8, 9, synth.TINY_ILENS[::-1], synth.TINY_YLENS[::-1], 14) + synth.batch(8, 9, [7, 10, 12], [2, 2, 2], 42)[:2]

    def steps(tag, sync_each, ms):
        solver, dev = TD._solver(str(tmp_path / tag), monkeypatch, synth.TINY, synth.TINY_LM, deterministic=True, pipeline_steps=6)
        torch.manual_seed(3)
        np.random.seed(4)
        data = [(torch.from_numpy(xs).to(dev), il, [torch.from_numpy(y).to(dev) for y in ys], torch.from_numpy(uxs).to(dev), uil)
                for xs, il, ys, uxs, uil in (b1, b2)]
        metas = [solver.gen_train_one_iteration(*data[0])]          # (one step first: the model's constants go up once)
        solver.flush()
        torch.cuda.synchronize()
        st = None if sync_each else A.stalled(None, ms)
        t0 = time.perf_counter()
        for d in data:
            metas.append(solver.gen_train_one_iteration(*d))
            if sync_each:
                torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        proved = None if st is None else st.proved()
        solver.flush()
        torch.cuda.synchronize()
        out = {"p/" + n: p.detach().clone() for n, p in solver.model.named_parameters()}
        out["metas"] = torch.tensor([[float(m[k]) for k in ("loss", "sup_loss", "unsup_loss")] for m in metas], dtype=torch.float64)
        return out, host_ms, proved

    steps("warm", True, A.MIN_MS)
    want, host_ms, _ = steps("base", True, A.MIN_MS)
    ms = A.stall_ms(host_ms)
    got, _, proved = steps("stalled", False, ms)
    n, bad = A.differing(got, want)
    print("async-invariance two-ssl-steps host %.2f stall %.0f proved %d words %d/%d" % (host_ms, ms, proved, n, bad))
    assert proved, "the stall had ended before both steps were enqueued: nothing is proven"
    assert bad == 0, "%d of %d words differ when two generator steps are in flight" % (bad, n)


# ------------------------------------------------------------------------------------------------- 8: the pipelined solver
def test_pipelined_solver_gives_the_same_bits_at_every_depth(hb, in_stream, tmp_path, monkeypatch):
    """6 supervised steps of a tiny Solver in deterministic mode at pipeline_steps 0, 1 and 6 (= PINNED_ROWS - 2): every
    reported loss and every parameter bit-identical.  At depth 1 and 6 a stall goes in front of the first step and is still
    running when the host returns from step `depth`: the pipeline really is that deep."""
    import test_deterministic_gpu as TD
    from solver import Solver
    assert Solver.PINNED_ROWS - 2 == 6
    batches = [synth.batch(8, 9, il, yl, 13 + i) for i, (il, yl) in enumerate(
        [(synth.TINY_ILENS, synth.TINY_YLENS), (synth.TINY_ILENS[::-1], synth.TINY_YLENS[::-1])] * 3)]
    results, host_ms = {}, None
    for depth in (0, 1, 6):
        solver, dev = TD._solver(str(tmp_path / ("depth%d" % depth)), monkeypatch, synth.TINY, synth.TINY_LM,
                                 deterministic=True, pipeline_steps=depth)
        torch.manual_seed(3)
        np.random.seed(4)
        hb.persist_clear_abort(dev)
        data = [(torch.from_numpy(xs).to(dev), ilens, [torch.from_numpy(y).to(dev) for y in ys]) for xs, ilens, ys in batches]
        losses = [solver.sup_train_one_iteration(*data[0], 1.0)]     # (warms the pools: part of every depth's run)
        solver.flush()
        torch.cuda.synchronize()
        st = A.stalled(None, A.stall_ms(host_ms)) if depth else None
        t0 = time.perf_counter()
        proved = None
        for i, (xs, ilens, ys) in enumerate(data):
            losses.append(solver.sup_train_one_iteration(xs, ilens, ys, 1.0))
            if st is not None and i + 1 == depth:
                proved = st.proved()
        if depth == 0:
            host_ms = (time.perf_counter() - t0) * 1e3
        solver.flush()
        torch.cuda.synchronize()
        assert not hb.persist_aborted(dev)
        out = {"p/" + n: p.detach().clone() for n, p in solver.model.named_parameters()}
        out["losses"] = torch.tensor([float(v) for v in losses], dtype=torch.float64)
        results[depth] = out
        if depth:
            n, bad = A.differing(out, results[0])
            print("async-invariance solver pipeline_steps=%d host %.2f stall %.0f proved %d words %d/%d"
                  % (depth, host_ms, st.ms, proved, n, bad))
            assert proved, "the stall had ended when the host returned from step %d: the pipeline was not %d deep" % (depth, depth)
            assert bad == 0, "pipeline_steps=%d: %d of %d words differ from pipeline_steps=0" % (depth, bad, n)
    assert len(set(results[0]["losses"].tolist())) == 7


# ------------------------------------------------------------------------------------------------- 9: the current stream
_OTHER = {}


def _other_stream():
    """A stream whose work does not queue up behind the default stream's.  The runtime multiplexes its streams onto a few
    hardware queues (4 by default) and a queue runs its packets in order: a stream that shares the default stream's queue
    waits behind the stall whatever the library does.  Found once per process: behind a short stall on the default stream a
    fill on the candidate must complete.  Candidates are tried one at a time, at most 5 (one more than there are queues),
    and only the one found ever runs the library's calls; none: the test fails."""
    if "s" not in _OTHER:
        tried = 0
        for _ in range(5):
            cand, tried = torch.cuda.Stream(), tried + 1
            flag = torch.zeros(1, device=DEV)
            torch.cuda.synchronize()
            st = A.stalled(torch.cuda.default_stream(), A.MIN_MS)
            with torch.cuda.stream(cand):
                flag.fill_(1.0)
            cand.synchronize()
            free = st.proved()
            torch.cuda.synchronize()
            if free:
                _OTHER["s"] = cand
                break
        print("async-invariance current-stream: candidate %d of 5 runs beside the default stream" % tried if "s" in _OTHER
              else "async-invariance current-stream: no stream of 5 runs beside the default stream")
    assert "s" in _OTHER, "no stream whose work runs while the default stream is stalled"
    return _OTHER["s"]


def _on_stream(hb, name, call):
    """The default stream stalled; `call` under another stream, its inputs prepared there.  After that stream's
    synchronize the outputs have the base bits and the default stream's stall has still not ended: nothing of the call
    went to the null stream."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with hb.deterministic(True):
        base = call()
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3              # (host AND GPU time: the other stream is waited for below)
    base = {k: A.words(v).copy() for k, v in base.items()}
    s = _other_stream()
    with torch.cuda.stream(s), hb.deterministic(True):       # (the stream's own memory pool: nothing new behind the stall)
        host = {k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in call().items()}
    torch.cuda.synchronize()
    st = A.stalled(torch.cuda.default_stream(), A.stall_ms(host_ms))
    with torch.cuda.stream(s), hb.deterministic(True):
        got = call()
        for k, v in got.items():                            # (into pinned memory made before the stall: copies on s, no
            host[k].copy_(v, non_blocking=True)             # staging by the runtime, and a wait for s alone below)
    s.synchronize()
    proved = st.proved()
    n, bad = A.differing(host, base)
    torch.cuda.synchronize()
    print("async-invariance current-stream %s host %.2f stall %.0f proved %d words %d/%d" % (name, host_ms, st.ms, proved, n, bad))
    assert bad == 0, "%s on a non-default stream: %d of %d words differ (a launch or an upload went to another stream)" % (name, bad, n)
    assert proved, "%s on a non-default stream waited for the default stream's stall" % name


def test_current_stream_linear(hb, in_stream):
    import ops
    g = torch.Generator().manual_seed(3)
    x, w, b, dy = torch.randn(37, 24, generator=g), torch.randn(20, 24, generator=g), torch.randn(20, generator=g), torch.randn(37, 20, generator=g)

    def call():
        xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
        y = ops.linear(xd, wd, bd, relu=True)
        y.backward(dy.to(DEV))
        return dict(y=y.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)
    _on_stream(hb, "linear", call)


def test_current_stream_ctc_loss_and_beam(hb, in_stream):
    import ops
    utts, _ = B.ctc_utts()
    beam_utts, _, _ = B.beam_utts("a")

    def loss():
        c = B.frames_batch(utts)
        buf = torch.from_numpy(c["buf"]).to(DEV).requires_grad_()
        nll = ops.ctc_loss(buf[:, :, :c["V"]], hb.to_device_i32(c["lens"], DEV), torch.from_numpy(c["labels"]).to(DEV), c["label_lens"])
        nll.backward(torch.from_numpy(c["g"]).to(DEV))
        return dict(nll=nll.detach(), dlogits=buf.grad)

    def beam():
        c = B.frames_batch(beam_utts)
        res = ops.ctc_beam(torch.from_numpy(c["buf"]).to(DEV)[:, :, :c["V"]], hb.to_device_i32(c["lens"], DEV), B.BEAM["a"]["K"])
        return dict(zip(B.MODE_OUTPUTS["plain"], res))
    _on_stream(hb, "ctc_loss", loss)
    _on_stream(hb, "ctc_beam", beam)


def test_current_stream_front_end(hb, in_stream):
    import test_augment_gpu as TAU
    from frontend import Frontend
    fe = Frontend(dict(TAU.FE_CFG, delta_order=1, speed_perturb=TAU.SPEEDS, **TAU._augment_cfg()))
    items = TAU._items(5, seed=8, dtype=np.int16)
    wave = np.concatenate([f for f, _ in items])
    offs = np.concatenate([[0], np.cumsum([len(f) for f, _ in items])]).tolist()
    aug = [(0, 1, 8000, 12.0), (-1, 0, 1499, 5.0), (2, -1, 0, 9.0), (-1, -1, 3, 20.0), (1, 2, 0, 7.5)]
    torch.cuda.synchronize()                                # (the banks and plans went to the device on the default stream)

    def call():
        xs, ilens = fe(torch.from_numpy(wave).to(DEV), offs, factor_index=[0, 2, 1, 0, 2], augment=aug)
        return dict(xs=xs)
    _on_stream(hb, "frontend", call)


@pytest.mark.parametrize("persistent", [False, True], ids=["per-step H=16", "persistent H=128"])
def test_current_stream_lstm(hb, in_stream, persistent):
    import test_poison_gpu as TPG
    if persistent:
        Bn, I, H, lens = 8, 16, 128, [48, 48, 45, 40, 33, 20, 9, 1]
        if not hb.USE_PERSIST:
            pytest.fail("the persistent kernels are switched off in this process")
    else:
        Bn, I, H, lens = 3, 8, 16, [9, 7, 4]
    c = TPG._lstm_inputs(2, Bn, max(lens), I, H, lens, 11)

    def call():
        return {k: v.detach() for k, v in TPG._lstm_run(hb, c, 2, lens, False, persistent).items()}
    _on_stream(hb, "lstm %s" % ("persistent H=128" if persistent else "per-step H=16"), call)
    assert not hb.persist_aborted(torch.device(DEV))

"""No kernel writes outside the buffers it is given (tests/guard.py; DESIGN "Guard bands").

Every case: the inputs come from the suite's case tables and are fenced (NaN bands where they are pure float data) and
snapshotted; the operator runs once outside a scope (the base result) and once inside guard.guarded(p) for p in ("one",
"zero"), where every torch.empty / zeros / full of the library AND of the case itself (the outputs and workspaces an
hb-level call is handed) is fenced.  Then, in this order: guard.check on every band; assert_frozen on the const inputs; the
guarded result against the base result, bit for bit (every operator here sums in a fixed order or runs in deterministic
mode, profiles/poison_coverage.txt; the default-path cases name their gate); Stats.unfenced == [] and at least one fenced
allocation.

EXACT WORKSPACES.  The hb-level functions are handed torch.empty((bytes + 3) // 4) float32 words of what *_ws_bytes says -
no ops._row_capacity rounding - forward and backward on the same workspace.  ops.ctc_align, ops.ctc_segment, ops.rnnt_align,
ops.ctc_beam and ops.gtc_nbest_graphs allocate exactly that themselves and are called as they are.  The transducer beams run
their loop at the hb level on separate exact tensors; hb.BeamTableLm gets exactly beam_tlm_ws_bytes; gemm_det is served from
an exact scratch placed in hb._det_ws_cache; the plan images (exactly *_plan_bytes) are fenced inputs; the persistent
scratch is allocated again inside the scope at the host's size (>= asr_persist_scratch_bytes).

The cases that run another module's whole parity check (_under_guard: decoder, pack helpers, prefix state, BeamSearch) and
the LSTM grid fence every buffer the library and the check allocate, but not the inputs those checks upload themselves.

One line per case on stdout (pytest -s), collected in profiles/guard_coverage.txt."""
import time

import numpy as np
import pytest
import torch

import batch_cases as B
import guard as G
import poison as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
_T0 = time.time()


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


@pytest.fixture(autouse=True)
def _clean_pools():
    import ops
    P.empty_pool()
    ops._ARENA.__init__()
    yield
    P.empty_pool()
    ops._ARENA.__init__()
    assert not hasattr(torch.empty, "__wrapped__"), "a guarded() scope is still open"


def _cpu(out):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items() if v is not None}


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(G._bits(a), G._bits(b))


def _case(name, build, gate=None):
    """build(fz) -> (fn, const): fz(tensor or array, nan=False) puts an input on the device inside a fence; fn() -> dict of
    device tensors; const: the inputs the operator declares const.  gate(out, base, what): for a default-path (atomic)
    operator, in place of the bit comparison."""
    total, base, n_bands = G.Stats(), None, 0
    for p in (None,) + G.INT_PATTERNS:
        P.empty_pool()
        ins = G.Stats()

        def fz(t, nan=False):
            t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
            return G.fence(t.to(DEV).contiguous(), nan=nan, int_pattern=p or "one", stats=ins)
        fn, const = build(fz)
        snap = G.frozen(*const)
        if p is None:
            st = G.Stats()
            out = _cpu(fn())
        else:
            with G.guarded(p) as st:
                out = _cpu(fn())
        what = "%s %s" % (name, p or "base")
        n_bands += G.check(st, ins)
        G.assert_frozen(snap, what)
        P.empty_pool()
        if p is None:
            base = out
            continue
        assert sorted(out) == sorted(base), what
        if gate is not None:
            gate(out, base, what)
        else:
            for k in out:
                assert _bits_equal(out[k], base[k]), "%s: %s differs from the unguarded run" % (what, k)
        assert st.unfenced == [], "%s: not fenced: %r" % (what, st.unfenced)
        assert st.n_allocs > 0, "%s: nothing was fenced - the case is vacuous" % what
        st.records = []
        total.merge(st)
    print("guard_coverage %-44s %s; %d bands checked; intact, const inputs unchanged, %s; module %.1f s"
          % (name, total.line(), n_bands, "inside the gate" if gate else "bit-identical", time.time() - _T0))
    return total


# ------------------------------------------------------------------------------------------------- the harness sees a store
def test_positive_control_four_bytes_into_the_back_band(hb):
    """A torch fill_ through an as_strided view that reaches one float into the back band of a fenced device tensor - owned
    memory, no faulty kernel: check reports 4 damaged bytes at the data's end, names the allocation, and a second buffer
    beside it is intact."""
    st = G.Stats()
    t = G.fence(torch.arange(33, dtype=torch.float32, device=DEV), nan=True, stats=st)
    u = G.fence(torch.arange(5, dtype=torch.int32, device=DEV), stats=st)
    assert t.is_cuda and t.data_ptr() % 256 == 0 and G.check(st) == 4
    t.as_strided((2,), (1,), t.storage_offset() + 32).fill_(7.0)             # element 32 (the last) and element 33 (the band)
    with pytest.raises(G.GuardError) as e:
        G.check(st)
    d, = e.value.damage
    assert (d.side, d.offset, d.nbytes, d.words[0]) == ("back", 132, 4, 0x40e00000) and d.record.shape == (33,)
    assert "test_guard_gpu.py:" in d.record.site and "back band" in str(e.value) and "data+132" in str(e.value)
    assert float(t[32]) == 7.0 and u.tolist() == [0, 1, 2, 3, 4]
    print("guard_coverage %-44s %s; %s" % ("positive control", st.line(), d.line()))


# ------------------------------------------------------------------------------------------------- lattice losses, exact
def _ctc_utts(V):
    """batch_cases.CTC_SHAPES at V: the table's own utterances at CTC_V, the same shapes and labels on new logits at 257."""
    utts, _ = B.ctc_utts()
    if V == B.CTC_V:
        return utts
    rs = np.random.RandomState(20240 + V)
    return [dict(u, z=(3.0 * rs.normal(0, 1, size=(u["z"].shape[0], V))).astype(np.float32)) for u in utts]


def _frames(fz, hb, utts, cols=B.EXTRA_COLS):
    c = B.frames_batch(utts, 0, cols)
    buf = fz(c["buf"], nan=True)
    labels = fz(c["labels"] if c["labels"].size else np.zeros(1, dtype=np.int64))
    return c, buf, fz(np.array(c["lens"], dtype=np.int32)), labels, fz(c["offsets"].astype(np.int32)), fz(c["g"], nan=True)


@pytest.mark.parametrize("V", [B.CTC_V, 257])
@pytest.mark.parametrize("family", ["ctc", "ctc_star", "gtc"])
def test_lattice_loss_forward_and_backward_in_an_exact_workspace(hb, family, V):
    """ctc_loss_fwd/bwd, ctc_star_loss_fwd/bwd and gtc_loss_fwd/bwd (the CTC lattice of every row as a graph) on
    batch_cases.CTC_SHAPES - a row on each of the wave, block and strided paths, (1, 0), (1, 1), the infeasible row - with
    ld = V + 3 and a workspace of exactly *_ws_bytes: nll, dlogits [B, T, V] contiguous (lddz = V), and the workspace the
    backward reads after the forward."""
    import gtc
    utts = _ctc_utts(V)

    def build(fz):
        c, buf, lens, labels, offs, g = _frames(fz, hb, utts)
        nB, T = buf.shape[:2]
        z = buf[:, :, :V]
        lmax = max(c["label_lens"])
        const = [buf, lens, labels, offs, g]
        if family == "ctc_star":
            pen = fz(np.full(nB, -1.5, dtype=np.float32), nan=True)
            const.append(pen)
        if family == "gtc":
            table = gtc.GraphBatch([gtc.Graph.ctc(list(u["y"]), V) for u in utts], list(range(nB))).to(torch.device(DEV))
            const += [getattr(table, k) for k in hb._GTC_DTYPES]

        def fn():
            nll = torch.full((nB,), float("nan"), device=DEV)
            dz = torch.full((nB, T, V), float("nan"), device=DEV)
            if family == "ctc":
                ws = torch.empty((hb.ctc_ws_bytes(nB, T, V, lmax) + 3) // 4, device=DEV)
                hb.ctc_loss_fwd(z, V + 3, lens, labels, offs, lmax, True, nll, ws)
                hb.ctc_loss_bwd(z, V + 3, lens, labels, offs, lmax, True, g, ws, dz, V)
            elif family == "ctc_star":
                ws = torch.empty((hb.ctc_star_ws_bytes(nB, T, V, lmax) + 3) // 4, device=DEV)
                hb.ctc_star_loss_fwd(z, V + 3, lens, labels, offs, lmax, pen, True, nll, ws)
                hb.ctc_star_loss_bwd(z, V + 3, lens, labels, offs, lmax, pen, True, g, ws, dz, V)
            else:
                ws = torch.empty((hb.gtc_ws_bytes(nB, T, V, table.max_nodes) + 3) // 4, device=DEV)
                hb.gtc_loss_fwd(z, V + 3, lens, table, True, nll, ws)
                hb.gtc_loss_bwd(z, V + 3, lens, table, True, g, ws, dz, V)
            assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(dz).all())
            for i, t in enumerate(c["lens"]):
                assert not bool(dz[i, t:].any())
            return dict(nll=nll, dlogits=dz)
        return fn, const
    _case("%s fwd+bwd exact ws V=%d" % (family, V), build)


@pytest.mark.parametrize("group", ["wave", "block", "strided"])
def test_graph_ctc_groups_in_an_exact_workspace(hb, group):
    """gtc_loss_fwd/bwd on the rows of test_gtc_gpu (V = 34): shared graphs, n-best tries, a confusion network, a hub of
    in-degree 79, 600 nodes - and the row without a path."""
    import gtc
    import test_gtc_gpu as TG
    V = 34
    rows = TG._rows(V, group, 100 + V)
    rs = np.random.RandomState(7 * V + len(group))
    nB, T = len(rows), max(t for t, _ in rows)
    zs = rs.normal(0, 1, size=(nB, T, V)).astype(np.float32)
    batch = TG._batch(dict(graphs=[g for _, g in rows]), range(nB))

    def build(fz):
        buf = np.full((nB, T, V + 3), np.nan, dtype=np.float32)
        for i, (t, _) in enumerate(rows):
            buf[i, :t, :V] = zs[i, :t]
        buf, lens = fz(buf, nan=True), fz(np.array([t for t, _ in rows], dtype=np.int32))
        g = fz(np.linspace(-2, 2, nB).astype(np.float32), nan=True)
        table = batch.to(torch.device(DEV))
        z = buf[:, :, :V]

        def fn():
            nll = torch.full((nB,), float("nan"), device=DEV)
            dz = torch.full((nB, T, V), float("nan"), device=DEV)
            ws = torch.empty((hb.gtc_ws_bytes(nB, T, V, table.max_nodes) + 3) // 4, device=DEV)
            hb.gtc_loss_fwd(z, V + 3, lens, table, True, nll, ws)
            hb.gtc_loss_bwd(z, V + 3, lens, table, True, g, ws, dz, V)
            assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(dz).all()) and float(nll[5]) == 0.0
            return dict(nll=nll, dlogits=dz)
        return fn, [buf, lens, g] + [getattr(table, k) for k in hb._GTC_DTYPES]
    _case("gtc fwd+bwd exact ws V=34 %s" % group, build)


def test_nbest_trie_built_on_the_device(hb):
    """ops.gtc_nbest_graphs at K = 8 (gtc_nbest_ref.random_lists): the capacity-sized table arrays, log_weights, dropped and
    the builder's int32 workspace of exactly asr_nbest_gtc_bytes; then the loss on the table in an exact workspace."""
    import gtc_nbest_ref as NR
    import ops
    nB, K, L, V = 4, 8, 12, 6
    hyp, hyp_len, score = NR.random_lists(np.random.RandomState(11), nB, K, L, V, share=0.4)
    T = 2 * L + 3
    zs = np.random.RandomState(12).normal(0, 1, size=(nB, T, V)).astype(np.float32)

    def build(fz):
        h, hl = fz(np.ascontiguousarray(hyp, dtype=np.int32)), fz(np.ascontiguousarray(hyp_len, dtype=np.int32))
        sc, z = fz(np.ascontiguousarray(score, dtype=np.float32)), fz(zs, nan=True)
        lens, g = fz(np.array([T, T - 1, T, 3], dtype=np.int32)), fz(np.ones(nB, dtype=np.float32), nan=True)

        def fn():
            table = ops.gtc_nbest_graphs(h, hl, sc, V)
            nll = torch.full((nB,), float("nan"), device=DEV)
            dz = torch.full((nB, T, V), float("nan"), device=DEV)
            ws = torch.empty((hb.gtc_ws_bytes(nB, T, V, table.max_nodes) + 3) // 4, device=DEV)
            hb.gtc_loss_fwd(z, V, lens, table, True, nll, ws)
            hb.gtc_loss_bwd(z, V, lens, table, True, g, ws, dz, V)
            out = dict(nll=nll, dlogits=dz, log_weights=table.log_weights, dropped=table.dropped, node_off=table.node_off)
            assert bool(torch.isfinite(nll).all())
            return out
        return fn, [h, hl, sc, z, lens, g]
    _case("gtc_nbest_graphs K=8 + gtc loss", build)


def test_rnnt_loss_and_joint_in_exact_buffers(hb):
    """rnnt_loss_fwd/bwd on batch_cases.RNNT_LATTICES with ld = V + 3 in a workspace of exactly rnnt_ws_bytes, and
    rnnt_joint_fwd/bwd into exact z, dpe, dpp."""
    utts, _ = B.rnnt_utts()

    def build(fz):
        c, j = B.rnnt_batch(utts, 0, B.EXTRA_COLS), B.joint_batch(utts)
        V, U, T, nB = c["V"], c["U"], c["T"], len(utts)
        buf, lens = fz(c["buf"], nan=True), fz(np.array(c["lens"], dtype=np.int32))
        labels = fz(c["labels"])
        offs = fz(np.concatenate([[0], np.cumsum(c["label_lens"])]).astype(np.int32))
        g, pe, pp, dzj = fz(c["g"], nan=True), fz(j["pe"], nan=True), fz(j["pp"], nan=True), fz(j["dz"], nan=True)
        z = buf[..., :V]

        def fn():
            nll = torch.full((nB,), float("nan"), device=DEV)
            dz = torch.full((nB, T, U + 1, V), float("nan"), device=DEV)
            ws = torch.empty((hb.rnnt_ws_bytes(nB, T, U, 4, V) + 3) // 4, device=DEV)
            hb.rnnt_loss_fwd(z, V + 3, lens, labels, offs, nll, ws)
            hb.rnnt_loss_bwd(z, V + 3, lens, labels, offs, g, ws, dz, V)
            zj = torch.full((nB, T, U + 1, B.RNNT_J), float("nan"), device=DEV)
            dpe, dpp = torch.full_like(pe, float("nan")), torch.full_like(pp, float("nan"))
            hb.rnnt_joint_fwd(pe, pp, lens, offs, zj)
            hb.rnnt_joint_bwd(dzj, zj, lens, offs, dpe, dpp)
            for t in (nll, dz, zj, dpe, dpp):
                assert bool(torch.isfinite(t).all())
            return dict(nll=nll, dlogits=dz, z=zj, dpe=dpe, dpp=dpp)
        return fn, [buf, lens, labels, offs, g, pe, pp, dzj]
    _case("rnnt loss fwd+bwd exact ws, joint fwd+bwd", build)


# ------------------------------------------------------------------------------------------------- aligners
def test_ctc_align_greedy_and_transducer_align(hb):
    """ops.ctc_align and ops.ctc_greedy on batch_cases.align_utts() (its row with fewer frames than labels included),
    ops.rnnt_align on RNNT_LATTICES: their workspaces are torch.empty of exactly *_align_ws_bytes."""
    import ops
    utts, _ = B.align_utts()
    rutts, _ = B.rnnt_utts()

    def build(fz):
        c, buf, lens, labels, offs, _ = _frames(fz, hb, utts)
        r = B.rnnt_batch(rutts, 0, B.EXTRA_COLS)
        rbuf, rlens, rlabels = fz(r["buf"], nan=True), fz(np.array(r["lens"], dtype=np.int32)), fz(r["labels"])

        def fn():
            a = ops.ctc_align(buf[:, :, :c["V"]], lens, labels[:c["labels"].size], c["label_lens"])
            ids, n, ftok = ops.ctc_greedy(buf[:, :, :c["V"]], lens)
            ra = ops.rnnt_align(rbuf[..., :r["V"]], rlens, rlabels, r["label_lens"])
            out = dict(path=a.path, score=a.score, first=a.first, last=a.last, token_logp=a.token_logp, ids=ids, n=n, ftok=ftok)
            out.update({"rnnt_" + k: getattr(ra, k) for k in ("score", "emit_frame", "token_logp", "frame_labels", "blank_logp")})
            return out
        return fn, [buf, lens, labels, rbuf, rlens, rlabels]
    _case("ctc_align, ctc_greedy, rnnt_align", build)


# ------------------------------------------------------------------------------------------------- searches
@pytest.mark.parametrize("mode", B.MODES)
def test_ctc_beam(hb, mode):
    """ops.ctc_beam on batch_cases.BEAM["a"] (V = 34, K = 4, lens 0, 1, 7, 100) in every mode: hyp, hyp_len, the scores and
    the workspace of exactly ctc_beam_ws_bytes."""
    import ops
    utts, _, fixtures = B.beam_utts("a")
    K = B.BEAM["a"]["K"]
    kw = B.beam_kwargs(mode, fixtures, utts, "base")

    def build(fz):
        c = B.frames_batch(utts, 0, B.EXTRA_COLS)
        buf, lens = fz(c["buf"], nan=True), fz(np.array(c["lens"], dtype=np.int32))

        def fn():
            with hb.deterministic(True):
                res = ops.ctc_beam(buf[:, :, :c["V"]], lens, K, **kw)
            return dict(zip(B.MODE_OUTPUTS[mode], res))
        return fn, [buf, lens]
    _case("ctc_beam %s (a)" % mode, build)


# ------------------------------------------------------------------------------------------------- scoring
def test_mwer_and_edit_distances(hb):
    """mwer_fwd / mwer_bwd on batch_cases.mwer_utts() with a workspace of exactly L R floats; edit_distance and
    word_edit_distance on batch_cases.edit_pairs() (a hypothesis at ED_MAX_COLS)."""
    utts, _ = B.mwer_utts()
    pairs, _ = B.edit_pairs(hb.ED_MAX_COLS)

    def build(fz):
        c = B.mwer_batch(utts, 0, B.EXTRA_COLS)
        nB, K, L, V = c["B"], c["K"], c["L"], c["V"]
        R = nB * K
        buf, tokens, npos, err = fz(c["buf"], nan=True), fz(c["tokens"]), fz(c["npos"]), fz(c["err"])
        gl = fz(np.array([B.MWER_G], dtype=np.float32), nan=True)
        pc = B.pairs_batch(pairs)
        hyp, ref, ref_len, hyp_len = fz(pc["hyp"]), fz(pc["ref"]), fz(pc["ref_len"]), fz(pc["hyp_len"])

        def fn():
            logits = buf[:, :, :V]
            o = {k: torch.full((R,), float("nan"), device=DEV) for k in ("seq_logp", "post", "coef")}
            risk, loss = torch.full((nB,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
            ws = torch.empty(L * R, device=DEV)
            hb.mwer_fwd(logits, tokens, npos, err, nB, B.MWER_SCALE, o["seq_logp"], o["post"], o["coef"], risk, loss, ws)
            dz = torch.full((L, R, V), float("nan"), device=DEV)
            hb.mwer_bwd(logits, tokens, npos, o["coef"], nB, gl, B.MWER_SCALE, dz)
            assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(loss).all())
            out = dict(o, risk=risk, loss=loss, dlogits=dz)
            for name, res in (("tok", hb.edit_distance(hyp, ref, ref_len, hyp_len=hyp_len)),
                              ("word", hb.word_edit_distance(hyp, ref, ref_len, B.ED_SPACE, hyp_len=hyp_len))):
                out.update({"%s_%s" % (name, k): v for k, v in zip(("dist", "hyp_n", "ref_n"), res)})
            return out
        return fn, [buf, tokens, npos, err, gl, hyp, ref, ref_len, hyp_len]
    _case("mwer fwd+bwd, edit_distance, word_edit_distance", build)


# ------------------------------------------------------------------------------------------------- GEMM and reductions
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", [(130, 80, 2051), (17, 130, 1000)])
def test_gemm(hb, M, N, K, ta, tb):
    """hb.gemm (plain, split 3, bias + relu: the default products meet in atomics, gate of test_hip_parity.test_gemm_variants
    against the unguarded run's float64-checked twin) and hb.gemm_det at split None and 7 (bit for bit), whose slabs live in
    hb._det_ws_cache of exactly gemm_det_split()["bytes"]."""
    import test_hip_parity as TP
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    Bm = torch.randn((N, K) if tb else (K, N), generator=g)
    bias = torch.randn(N, generator=g)
    ref = (A.double().t() if ta else A.double()) @ (Bm.double().t() if tb else Bm.double())

    def build(fz):
        a, b, bd = fz(A, nan=True), fz(Bm, nan=True), fz(bias, nan=True)

        def fn():
            return dict(plain=hb.gemm(a, b, trans_a=ta, trans_b=tb), split3=hb.gemm(a, b, trans_a=ta, trans_b=tb, split_k=3),
                        epilogue=hb.gemm(a, b, trans_a=ta, trans_b=tb, bias=bd, relu=True),
                        det=hb.gemm_det(a, b, trans_a=ta, trans_b=tb), det7=hb.gemm_det(a, b, trans_a=ta, trans_b=tb, split=7))
        return fn, [a, b, bd]

    def gate(out, base, what):
        gg = dict(rtol=TP.GEMM_ARITH[0][1], atol=TP.GEMM_ATOL)
        for k in ("plain", "split3", "det", "det7"):
            TP._close(out[k], ref.float(), what=what + " " + k, **gg)
        TP._close(out["epilogue"], torch.relu(ref + bias).float(), what=what + " bias+relu", **gg)
        for k in ("det", "det7"):
            assert _bits_equal(out[k], base[k]), what + " " + k
    _case("gemm, gemm_det %dx%dx%d %s%s" % (M, N, K, "T" if ta else "N", "T" if tb else "N"), build, gate=gate)


def _exact_det_scratch(hb, nbytes):
    """The ordered reductions' scratch (hb._det_ws_cache, which hb.det_workspace grows by 1024 words above the request) as a
    tensor of exactly (nbytes + 3) // 4 words under the cache's own key for this device and stream: the next ordered call
    that asks for at most nbytes is served from it."""
    hb._det_ws_cache.clear()
    hb.det_workspace(torch.device(DEV), 4)
    key, = hb._det_ws_cache
    ws = hb._det_ws_cache[key] = torch.empty((int(nbytes) + 3) // 4, device=DEV)
    return ws


@pytest.mark.parametrize("split", [None, 7])
def test_gemm_det_in_a_scratch_of_exactly_gemm_det_ws_bytes(hb, split):
    """hb.gemm_det at 130 x 80 x 2051 (TN: the weight-gradient form) and 17 x 130 x 1000 (NN) with its slabs in a scratch of
    exactly asr_gemm_det_ws_bytes (gemm_det_split()["bytes"]), not the 1024 words more that the cache allocates."""
    g = torch.Generator().manual_seed(5)
    Ah, Bh = torch.randn(2051, 130, generator=g), torch.randn(2051, 80, generator=g)
    Ch, Dh = torch.randn(17, 1000, generator=g), torch.randn(1000, 130, generator=g)
    need1 = hb.gemm_det_split(130, 80, 2051, trans_a=True, split=split)
    need2 = hb.gemm_det_split(17, 130, 1000, split=split)
    assert need1["rc"] == 0 and need1["split"] > 1 and need1["bytes"] > 0 and need2["rc"] == 0

    def build(fz):
        a, b, c, d = fz(Ah, nan=True), fz(Bh, nan=True), fz(Ch, nan=True), fz(Dh, nan=True)

        def fn():
            out = {}
            for name, x, y, ta, need in (("tn", a, b, True, need1), ("nn", c, d, False, need2)):
                ws = _exact_det_scratch(hb, need["bytes"]) if need["bytes"] else None
                out[name] = hb.gemm_det(x, y, trans_a=ta, split=split)
                if ws is not None:
                    key, = hb._det_ws_cache
                    assert hb._det_ws_cache[key] is ws and ws.numel() * 4 - need["bytes"] < 4, "the call was not served from it"
            return out
        return fn, [a, b, c, d]
    _case("gemm_det exact scratch split %s" % split, build)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("n", [1, 3, 8197])
def test_reductions(hb, n, det):
    """hb.colsum over [n, 260] (a strided view of 263 columns), hb.colsum_parts over three parts of n rows, hb.sumsq over n,
    hb.gather_sumsq of seven sources with n among them into an exact flat buffer - on the default path (atomics: the gates of
    test_gemm_skinny_and_colsum, rtol 1e-5 + 1e-4, and of test_gather_sumsq_kernel, 1e-5 of the sum, against float64) and in
    deterministic mode (the same gates, and bit for bit) - and hb.gemm_skinny / hb.gemm_side (mask 0xf0) inside the gate of
    test_gemm_side_on_a_subset_of_the_xcds."""
    import test_hip_parity as TP
    g = torch.Generator().manual_seed(9 + n)
    Xh = torch.randn(n, 263, generator=g)
    xh = torch.randn(n, generator=g)
    parth = [torch.randn(n, 5, generator=g), torch.randn(n, 3, 7, generator=g), torch.randn(n, 1, generator=g)]
    sizes = [1, 3, 4, 5, n, 33, 7]
    srch = [torch.randn(s, generator=g) for s in sizes]
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off += (s + 3) // 4 * 4
    Ah, Bh = torch.randn(2051, 130, generator=g), torch.randn(2051, 80, generator=g)
    Sh, Wh = torch.randn(3, 32, generator=g), torch.randn(9, 32, generator=g)      # (test_gemm_skinny_and_colsum's 3 x 9 x 32)

    def build(fz):
        X, x, srcs = fz(Xh, nan=True), fz(xh, nan=True), [fz(s, nan=True) for s in srch]
        parts = [fz(t, nan=True) for t in parth]
        a, b, s_, w = fz(Ah, nan=True), fz(Bh, nan=True), fz(Sh, nan=True), fz(Wh, nan=True)

        def fn():
            with hb.deterministic(det):
                flat = torch.empty(off, device=DEV)
                acc = torch.zeros(1, device=DEV)
                hb.gather_sumsq(srcs, offs, flat, acc)
                out = dict(colsum=hb.colsum(X[:, :260]), sumsq=hb.sumsq(x, torch.zeros(1, device=DEV)), gathered_sumsq=acc,
                           gathered=torch.cat([flat[o:o + k] for o, k in zip(offs, sizes)]))
                out.update({"part%d" % i: t for i, t in enumerate(hb.colsum_parts(parts))})
            side, queue = torch.zeros(130, 80, device=DEV), torch.zeros(1, device=DEV)
            assert hb.gemm_side(a, b, side, queue, 0xf0, trans_a=True)
            out.update(side=side, skinny=hb.gemm_skinny(s_, w))
            return out
        return fn, [X, x, a, b, s_, w] + srcs + parts

    def gate(out, base, what):
        gg = dict(rtol=TP.GEMM_ARITH[0][1], atol=TP.GEMM_ATOL)
        TP._close(out["side"], (Ah.double().t() @ Bh.double()).float(), what=what + " side", **gg)
        TP._close(out["skinny"], (Sh.double() @ Wh.double().t()).float(), what=what + " skinny", **gg)
        TP._close(out["colsum"], Xh[:, :260].double().sum(0).float(), what=what + " colsum", **gg)
        for i, t in enumerate(parth):
            TP._close(out["part%d" % i], t.double().sum(0).float(), what=what + " colsum_parts %d" % i, **gg)
        want = float((xh.double() ** 2).sum())
        assert abs(float(out["sumsq"]) - want) <= 1e-5 * want, what + " sumsq"
        want = sum(float((t.double() ** 2).sum()) for t in srch)
        assert abs(float(out["gathered_sumsq"]) - want) <= 1e-5 * want, what + " gather_sumsq"
        assert torch.equal(out["gathered"], torch.cat(srch)), what
        if det:
            for k in out:
                if k not in ("side", "skinny"):
                    assert _bits_equal(out[k], base[k]), what + " " + k
    _case("colsum, colsum_parts, sumsq, gather_sumsq %s, gemm_side, gemm_skinny n=%d" % ("det" if det else "default", n),
          build, gate=gate)


# ------------------------------------------------------------------------------------------------- sequence kernels
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("persistent", [False, True])
def test_lstm_layer(hb, persistent, packed, det):
    """ops.lstm_layer forward and backward, both directions: per-step H = 16, B = 3, T = 9 and persistent H = 128, B = 8,
    T = 48 ragged, padded and packed, default and deterministic (test_poison_gpu.test_lstm_layer's grid; its inputs, runner
    and - on the default path, whose weight gradients meet in atomics - its gate against the float64 oracle).  The pooled
    workspace, the gate and state buffers and every gradient are fenced."""
    import test_poison_gpu as TPG
    if persistent:
        nB, I, H, lens = 8, 16, 128, [48, 48, 45, 40, 33, 20, 9, 1]
        if not hb.USE_PERSIST:
            pytest.fail("the persistent kernels are switched off in this process")
    else:
        nB, I, H, lens = 3, 8, 16, [9, 7, 4]
    c = TPG._lstm_inputs(2, nB, max(lens), I, H, lens, 11)

    oracle_gate, _ = TPG._lstm_gate(c, lens, packed, hb)

    def build(fz):
        def fn():
            if persistent:
                # the persistent kernels' control block and exchange area (one torch.zeros of 128 bytes +
                # asr_persist_scratch_bytes, kept for the life of the process): allocated again, so that a guarded run fences
                # it; it comes back zeroed, which is the state the kernels expect between launches
                torch.cuda.synchronize()
                hb._persist_scratch.pop(hb._scratch_key(torch.device(DEV)), None)
            with hb.deterministic(det):
                out = TPG._lstm_run(hb, c, 2, lens, packed, persistent)
            out.pop("pad_rows", None)
            return out
        return fn, []
    _case("lstm %s %s %s" % ("persistent H=128 T=48" if persistent else "per-step H=16 T=9", "packed" if packed else "padded",
                             "deterministic" if det else "default"), build,
          gate=None if det else lambda out, base, what: oracle_gate(out, what))


def test_pyramid_concat_and_rows(hb):
    """ops.pyramid_concat at odd T = 11 and T = 1 (mask tensor, seeded mask, none), hb.rows_pack, ops.rows_unpack forward
    and backward with relu(fill) and a seeded mask."""
    import ops
    g = torch.Generator().manual_seed(7)
    T, nB, C, lens = 11, 3, 8, [11, 7, 4]
    xh = torch.randn(T, nB, C, generator=g)
    maskh = (torch.rand(T, nB, C, generator=g) > 0.3).float() / 0.7
    dyh = torch.randn((T + 1) // 2, nB, 2 * C, generator=g)
    xbh = torch.randn(nB, T, C, generator=g)
    for b_, n_ in enumerate(lens):
        xbh[b_, n_:] = 0.0
    fillh, douth = torch.randn(C, generator=g), torch.randn(nB, T, C, generator=g)

    def build(fz):
        x, mask, dy, xb, fill, dout = (fz(t, nan=True) for t in (xh, maskh, dyh, xbh, fillh, douth))
        layout = hb.RowLayout(lens, [], DEV)
        rows = hb.LayerRows(layout, 0)

        def fn():
            out = {}
            with hb.deterministic():
                for name, m in (("mask", mask), ("seeded", hb.SeededMask((T, nB, C), 0.3, DEV, seed=99)), ("plain", None)):
                    xg = x.detach().requires_grad_()
                    y = ops.pyramid_concat(xg, m)
                    y.backward(dy)
                    out.update({"pyr_%s_y" % name: y, "pyr_%s_dx" % name: xg.grad})
                x1 = x[:1].detach().contiguous().requires_grad_()
                y1 = ops.pyramid_concat(x1, None)
                y1.backward(dy[:1].contiguous())
                out.update(pyr_T1_y=y1, pyr_T1_dx=x1.grad)
                packed = hb.rows_pack(xb, rows)
                out["packed"] = packed
                for name, m in (("plain", None), ("seeded", hb.SeededMask((nB, T, C), 0.3, DEV, seed=5))):
                    pk, fl = packed.detach().clone().requires_grad_(True), fill.detach().requires_grad_(True)
                    u = ops.rows_unpack(pk, rows, T, fl, m, True)
                    u.backward(dout)
                    out.update({"unpack_%s" % name: u, "unpack_%s_drows" % name: pk.grad, "unpack_%s_dfill" % name: fl.grad})
            return out
        return fn, [x, mask, dy, xb, fill, dout]
    _case("pyramid_concat T=11, T=1, rows_pack, rows_unpack", build)


def test_label_logprob(hb):
    """ops.label_logprob forward and backward with the sum and the argmax (L = 5, B = 7, V = 34; test_poison_gpu's case) in
    deterministic mode."""
    import ops
    L, nB, V = 5, 7, 34
    g = torch.Generator().manual_seed(L + V)
    logits, idx = torch.randn(L, nB, V, generator=g) * 3, torch.randint(0, V, (L, nB), generator=g)
    dist = torch.rand(V, generator=g)
    dist = dist / dist.sum()
    go = torch.randn(L, nB, generator=g)

    def build(fz):
        ld, id_, dd, god = fz(logits, nan=True), fz(idx), fz(dist, nan=True), fz(go, nan=True)

        def fn():
            with hb.deterministic(True):
                z = ld.detach().requires_grad_()
                out, total, amax = ops.label_logprob(z, id_, dd, 0.05, with_sum=True, sum_scale=-1.0 / (L * nB), with_argmax=True)
                ((out * god).sum() + 2.0 * total).backward()
                return dict(out=out, total=total.reshape(1).clone(), argmax=amax, dz=z.grad)
        return fn, [ld, id_, dd, god]
    _case("label_logprob sum + argmax deterministic", build)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return _bits_equal(a.cpu(), b.cpu())
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _under_guard(name, check):
    """check() runs an operator AND its existing parity check (inputs, reference and gate are that test's own, imported) ->
    its outputs or None.  Run unguarded, then under both patterns: every buffer the operator and the check allocate with
    torch.empty & co is fenced (the inputs such a check uploads with .to() are not: the cases above fence theirs).  Bands
    first, then the outputs where check returns them, bit for bit."""
    total, n_bands = G.Stats(), 0
    P.empty_pool()
    base = check()
    torch.cuda.synchronize()
    for p in G.INT_PATTERNS:
        P.empty_pool()
        with G.guarded(p) as st:
            got = check()
        n_bands += G.check(st)
        assert _same(base, got), "%s %s: the outputs differ from the unguarded run's" % (name, p)
        assert st.unfenced == [], "%s %s: not fenced: %r" % (name, p, st.unfenced)
        assert st.n_allocs > 0, "%s %s: nothing was fenced - the case is vacuous" % (name, p)
        st.records = []
        total.merge(st)
        P.empty_pool()
    print("guard_coverage %-44s %s; %d bands checked; intact, inside the operator's own parity check%s; module %.1f s"
          % (name, total.line(), n_bands, "" if base is None else ", bit-identical", time.time() - _T0))


@pytest.mark.parametrize("name", ["C10-T60-K1", "smooth-V37-C10-T60-K100", "greedy-V37-C8-T128-K100"])
def test_decoder_sequence(hb, name, monkeypatch):
    """ops.decoder_sequence forward and backward through the whole check of test_decoder_shapes_gpu (persistent both ways;
    per-step backward with dec_feedback_bwd; greedy): hb.DecBuffers, dec_prepare, the saved-for-backward stores and every
    gradient are fenced.  The float64 reference is computed once."""
    import test_decoder_shapes_gpu as TDS
    case = [c.values[0] for c in TDS.TEACHER_CASES + TDS.FREE_CASES if c.values[0]["name"] == name]
    assert len(case) == 1, name
    cache, reference = {}, TDS._reference

    def once(c, x, dtype):
        key = (c["name"], dtype)
        if key not in cache:
            with torch.random.fork_rng():
                cache[key] = reference(c, x, dtype)
        return cache[key]
    monkeypatch.setattr(TDS, "_reference", once)
    _under_guard("decoder_sequence " + name, lambda: TDS._case(case[0]))


def test_prefix_state_beam_search_and_transducer_beams(hb):
    """hb.CtcPrefixState init + 4 x score / advance (V = 34, T' = 100, K = 4); hb.BeamSearch select at K = 4, V = 33 with and
    without the LM, reorder, and whole searches with the backtrack; the transducer beam search and the word beam at the
    smallest case of their grids: each through its own module's check."""
    import rnnt_beam_ref as BR
    import rnnt_wbeam_ref as WB
    import test_beam_ctc_gpu as TBC
    import test_beam_gpu as TB
    import test_rnnt_beam_gpu as TRB
    import test_rnnt_wbeam_gpu as TRW
    _under_guard("CtcPrefixState init, 4 x score + advance", lambda: TBC._report("guarded V=34 T'=100 K=4", TBC._kernel_case(hb, 34, 100, 4, 3.0)))
    _under_guard("BeamSearch.select K=4 V=33", lambda: (TB.test_select_kernel_against_a_stable_sort(hb, 4, 33, False),
                                                        TB.test_select_kernel_against_a_stable_sort(hb, 4, 33, True))[0])
    _under_guard("BeamSearch.reorder", lambda: TB.test_reorder_is_an_exact_permutation(hb))
    _under_guard("BeamSearch select, reorder, backtrack K=4 B=5", lambda: TB.test_beams_against_the_float64_restatement(hb, 4, 320, 128, 30, 5))
    _under_guard("rnnt_beam %r" % (BR.GRID[0],), lambda: TRB.test_grid(hb, *BR.GRID[0]))
    _under_guard("rnnt_wbeam %s" % WB.grid_id(WB.GRID[0]), lambda: TRW.test_grid(hb, WB.GRID[0]))


def _rnnt_beam_exact(hb, head, x, lens, K, L, word_lm=None, **kw):
    """ops.rnnt_beam's loop (init; T' + L iterations of step, gate product, cell, projection; backtrace) at the hip_backend
    level with the workspace, the state h / c / xh / gates / pp and the word beam's extra workspace as SEPARATE tensors of
    exactly the advertised sizes - ops cuts them from one pooled buffer that is rounded up."""
    pe = head.project_enc(x).detach().contiguous()
    nB, T, J = pe.shape
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in head.lstm.direction_params(0))
    w_gate, b_gate = torch.cat([w_ih, w_hh], dim=1).contiguous(), (b_ih + b_hh).contiguous()
    w_pred, w_out, b_out, emb = (t.detach().contiguous() for t in (head.lin_pred.weight, head.lin_out.weight, head.lin_out.bias,
                                                                  head.embedding.weight))
    V, E, P = w_out.shape[0], emb.shape[1], w_pred.shape[1]
    f32, i32 = dict(device=DEV, dtype=torch.float32), dict(device=DEV, dtype=torch.int32)
    ws = torch.empty((hb.rnnt_beam_ws_bytes(nB, T, J, V, K, L, E, P) + 3) // 4, **f32)
    h, c, xh, gates, pp = (torch.empty(nB * K, n, **f32) for n in (P, P, E + P, 4 * P, J))
    args = (pe, w_out, b_out, emb, lens, K, L, h, c, xh, pp, ws)
    if word_lm is not None:
        wws = torch.empty((hb.rnnt_wbeam_ws_bytes(nB, K) + 3) // 4, **i32)
        run = hb.RnntWordBeam(*args, word_lm.to(torch.device(DEV)), wws, kw["word_lm_weight"], kw["word_bonus"], kw["eos_term"],
                              kw["lexicon_only"])
    else:
        run = hb.RnntBeam(*args)
    run.init(head.bos)
    for it in range(T + L + 1):
        if it > 0:
            run.step(it - 1)
            if it == T + L:
                break
        run.product(xh, w_gate, gates, b_gate)
        run.cell(gates)
        run.product(h, w_pred, pp)
    hyp, hyp_len, score = torch.empty(nB, K, L, **i32), torch.empty(nB, K, **i32), torch.empty(nB, K, **f32)
    if word_lm is None:
        run.backtrace(hyp, hyp_len, score)
        return dict(hyp=hyp, hyp_len=hyp_len, score=score)
    rs, lm, nw = torch.empty_like(score), torch.empty_like(score), torch.empty_like(hyp_len)
    run.backtrace(hyp, hyp_len, score, rs, lm, nw)
    return dict(hyp=hyp, hyp_len=hyp_len, score=score, rnnt_score=rs, lm_score=lm, n_words=nw)


@pytest.mark.parametrize("kind", ["beam", "word_beam"])
def test_transducer_beams_in_exact_workspaces(hb, kind):
    """The transducer beam search (rnnt_beam_ref.GRID[2]: V = 3, K = 4, J = 32, frames 7, 0, 2) and the word beam
    (rnnt_wbeam_ref.GRID[1]: V = 5, K = 4, J = 32) at the hip_backend level in workspaces of exactly
    asr_transducer_beam_ws_bytes and asr_transducer_wbeam_ws_bytes; the result equals head.beam's (ops.rnnt_beam on the pooled
    buffer) bit for bit."""
    import rnnt_beam_ref as BR
    import rnnt_wbeam_ref as WB
    import test_rnnt_beam_gpu as TRB
    import test_rnnt_wbeam_gpu as TRW
    if kind == "beam":
        V, K, J, lens, L, seed = BR.GRID[2]
        (p, utts), kw, wlm = BR.grid_utterances(V, K, J, lens, L, seed), {}, None
    else:
        g = WB.GRID[1]
        V, K, J, L = g[0], g[1], g[2], g[4]
        p, utts, wlm = WB.grid_case(*g)
        kw = TRW._wkw(wlm, eos_term=g[7], lexicon_only=g[6])
    head = TRB._head(p)
    T = max(max(u.shape[0] for u in utts), 1) + 1
    xh_ = np.full((len(utts), T, utts[0].shape[1]), np.nan, np.float32)
    for b, u in enumerate(utts):
        xh_[b, :u.shape[0]] = u

    def build(fz):
        x, lens_d = fz(xh_, nan=True), fz(np.array([u.shape[0] for u in utts], dtype=np.int32))

        def fn():
            with torch.no_grad():
                out = _rnnt_beam_exact(hb, head, x, lens_d, K, L, **kw)
                want = head.beam(x, lens_d, K, L, **kw)
            for k, w in zip(out, want):
                assert _bits_equal(out[k].cpu(), w.cpu()), "%s: %s differs from ops.rnnt_beam" % (kind, k)
            return out
        return fn, [x, lens_d]
    _case("rnnt %s exact ws" % kind, build)


def test_attention_beam_with_ngram_and_word_lm_states(hb):
    """hb.BeamSearch with hb.BeamTableLm inside - the n-gram automaton and the word LM with its lexicon: one select at K = 4,
    V = 33 against test_beam_ngram_gpu's stable sort (its extra workspace is a tensor of exactly asr_beam_tlm_ws_bytes), and
    whole searches - init, every select and reorder, the backtrack - against the float64 restatement, where ops allocates
    the extra workspace at exactly that size."""
    import beam_ngram_ref as R
    import test_beam_ngram_gpu as TBN
    for kind in (R.NGRAM, R.WORD):
        _under_guard("BeamSearch + BeamTableLm select K=4 V=33 %s" % kind,
                     lambda: TBN.test_select_against_a_stable_sort_bit_for_bit(hb, 4, 33, kind, False))
    for key in [[k for k in R.grid() if k[0] == kind and k[2] == 4][0] for kind in (R.NGRAM, R.WORD)]:
        _under_guard("attention beam search + table LM %s" % (key,), lambda: TBN._check_search(hb, key))


def test_pack_helpers_feedback_and_embedding_grad(hb):
    """lstm_pack / unpack / unpack2, pack_multi, cell_pack, dec_pack with colsum_parts, dec_prepare, dec_feedback fwd / bwd,
    seeded dropout and the pad-fill gradient: the checks of test_hip_parity and test_deterministic_gpu at their smallest
    cases."""
    import test_deterministic_gpu as TD
    import test_hip_parity as TP
    _under_guard("lstm_pack, unpack, unpack2 H=16", lambda: TP.test_lstm_pack_unpack_roundtrip(16, 12, 2))
    _under_guard("lstm_pack_multi ndir=1", lambda: TP.test_lstm_pack_multi_equals_per_layer(1, [(20, 8), (20, 20)]))
    _under_guard("cell_pack", lambda: TP.test_cell_pack_unpack_roundtrip())
    _under_guard("dec_pack, colsum_parts", lambda: TP.test_dec_pack_and_colsum_parts(20, 12, 4, 36, 5))
    _under_guard("dec_prepare", lambda: (TP.test_dec_prepare_matches_torch(False), TP.test_dec_prepare_matches_torch(True))[0])
    _under_guard("dec_feedback fwd+bwd B=5 V=7", lambda: TP.test_decoder_feedback_kernels(5, 7, 12, 40))
    _under_guard("seeded dropout p=0.3 (pyramid seeded, relu bwd)", lambda: TP.test_seeded_dropout_kernels(0.3))
    _under_guard("rows_unpack_bwd relu_of + seeded mask", lambda: TD.test_pad_fill_grad_det(hb, 8, True, True))


@pytest.mark.parametrize("det", [False, True])
def test_embedding_grad(hb, det):
    """hb.embedding_grad at rows = 37, E = 16, V = 12, KX = 48 (test_embedding_grad_kernel's small case): demb [V, E]
    accumulates in place into a fenced copy; the row-strided gradient and the tokens (-1 among them) are const.  Default:
    that test's gate (rtol 1e-5, atol 1e-5) against index_add_ in float64; deterministic: bit for bit as well."""
    import test_hip_parity as TP
    rows, E, V, KX = 37, 16, 12, 48
    g = torch.Generator().manual_seed(rows + V)
    bufh = torch.randn(rows, KX, generator=g)
    tokh = torch.randint(0, V, (rows,), generator=g)
    tokh[torch.rand(rows, generator=g) < 0.2] = -1
    acch = torch.randn(V, E, generator=g)
    want = acch.double()
    want.index_add_(0, tokh[tokh >= 0], bufh[:, KX - E:][tokh >= 0].double())

    def build(fz):
        buf, tok, acc0 = fz(bufh, nan=True), fz(tokh), fz(acch, nan=True)

        def fn():
            acc = torch.empty_like(acc0).copy_(acc0)
            with hb.deterministic(det):
                assert hb.embedding_grad(tok, buf[:, KX - E:], acc)
            return dict(demb=acc)
        return fn, [buf, tok, acc0]

    def gate(out, base, what):
        TP._close(out["demb"], want.float(), rtol=1e-5, atol=1e-5, what=what)
        assert not det or _bits_equal(out["demb"], base["demb"]), what
    _case("embedding_grad rows=37 %s" % ("deterministic" if det else "default"), build, gate=gate)


def test_ctc_segment(hb):
    """ops.ctc_segment on the first case of ctc_segment_cases.GRID with free ends (V = 34, small): its outputs and the
    workspace of exactly ctc_segment_ws_bytes."""
    import ctc_segment_cases as SC
    import ops
    c = SC.case([g for g in SC.GRID if g[0] == 34 and g[1] == "small" and g[3] == 1][0])
    V, recs = c["V"], c["recs"]
    nB, T = c["z"].shape[0], c["z"].shape[1]
    z = np.asarray(c["z"], dtype=np.float32)
    bufh = np.full((nB, T, V + 3), np.nan, dtype=np.float32)
    for i, (t, _) in enumerate(recs):
        bufh[i, :t, :V] = z[i, :t]

    def build(fz):
        buf, lens = fz(bufh, nan=True), fz(np.array([t for t, _ in recs], dtype=np.int32))
        ys = fz(np.array([v for _, us in recs for u in us for v in u], dtype=np.int64))

        def fn():
            res = ops.ctc_segment(buf[:, :, :V], lens, ys, [[len(u) for u in us] for _, us in recs],
                                  free_ends=bool(c["free_ends"]), window=c["window"])
            return {k: getattr(res, k) for k in ("path", "score", "first", "last", "token_logp", "utt_begin", "utt_end",
                                                 "utt_logp", "utt_conf")}
        return fn, [buf, lens, ys]
    _case("ctc_segment V=34 small free ends", build)


# ------------------------------------------------------------------------------------------------- optimizer, dropout
def test_adam_clip_and_seeded_dropout(hb):
    """asr_adam_clip_f32 on flat buffers of exactly 8197 elements (p, m, v, vmax in place; g const; the norm word and the
    zero word one float each), and the seeded dropout kernels at n = 4 and 8196: the mask, the in-place product and the
    relu-dropout backward."""
    n = 8197
    g = torch.Generator().manual_seed(41)
    ph, gh = torch.randn(n, generator=g), torch.randn(n, generator=g)
    mh, vh = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
    xs = {k: torch.randn(k, generator=g) for k in (4, 8196)}

    def build(fz):
        p, gr, m, v, vmax = fz(ph, nan=True), fz(gh, nan=True), fz(mh, nan=True), fz(vh, nan=True), fz(vh * 1.5, nan=True)
        xd = {k: fz(x, nan=True) for k, x in xs.items()}

        def fn():
            with hb.deterministic(True):                     # (the ordered sum: the word feeds the clip factor of every p)
                word = hb.sumsq(gr, torch.zeros(1, device=DEV))
            zero_word = torch.full((1,), 3.0, device=DEV)
            rc = hb.load().asr_adam_clip_f32(n, hb.ptr(p), hb.ptr(gr), hb.ptr(m), hb.ptr(v), hb.ptr(vmax), hb.ptr(word), 5.0,
                                             5e-4, 0.9, 0.999, 1e-8, 1e-6, 1.0 - 0.9, 1.0 - 0.999, None, hb.ptr(zero_word),
                                             hb.stream())
            assert rc == 0, rc
            out = dict(p=p, m=m, v=v, vmax=vmax, word=word, zero_word=zero_word)
            for k, x in xd.items():
                mk = hb.SeededMask((k,), 0.3, DEV, seed=1234 + k)
                y = hb.dropout_seeded_(torch.relu(x).contiguous(), mk)
                out.update({"mask%d" % k: mk.tensor(), "y%d" % k: y, "dx%d" % k: hb.relu_dropout_bwd(x, y, mk.seed, mk.p)})
            return out
        return fn, [gr] + list(xd.values())
    _case("adam_clip n=8197, seeded dropout n=4, 8196", build)


# ------------------------------------------------------------------------------------------------- the front end
def test_front_end(hb):
    """batch_cases.waves() packed at odd offsets through Frontend.run (fbank, CMVN statistics and finish, deltas 2),
    hb.resample at SPEEDS, hb.reverb and hb.noise_mix, each into an exact output buffer."""
    from frontend import Frontend
    rows, _, banks = B.waves()
    fe = Frontend(dict(B.FE_CFG))
    plan, rplan, bank = hb.ResamplePlan(16000, B.SPEEDS), hb.ReverbPlan(banks["rirs"]), hb.NoiseBank(banks["clips"])

    def build(fz):
        c = B.waves_batch(rows, 0)
        samples, offsets = fz(c["samples"], nan=True), fz(c["offsets"])
        frames = [fe.num_frames(n) for n in c["lens"]]
        olens = [plan.out_samples(n, w["factor"]) for n, w in zip(c["lens"], rows)]
        ooffs = np.concatenate([[0], np.cumsum(olens)]).astype(np.int64)
        fr, fac, oo = fz(np.array(frames, dtype=np.int32)), fz(np.array([w["factor"] for w in rows], dtype=np.int32)), fz(ooffs)
        rir, clip = (fz(np.array([w[k] for w in rows], dtype=np.int32)) for k in ("rir", "clip"))
        start = fz(np.array([w["start"] for w in rows], dtype=np.int64))
        scale = fz(np.array([w["scale"] for w in rows], dtype=np.float32), nan=True)
        total = int(c["offsets"][-1])
        # the plans' device images, exactly asr_fbank_plan_bytes and asr_resample_plan_bytes long (asserted below): read-only
        # tables of the kernels, placed where plan.on(device) looks for them
        fplan, rtab = fz(fe.plan.words), fz(plan.tables, nan=True)
        assert fplan.numel() * 4 == hb.fbank_plan_bytes(fe.plan.n_fft) and rtab.numel() * 4 == hb.resample_plan_bytes(plan.geometry)
        fe.plan._dev = {str(fplan.device): fplan}
        plan._dev = {str(rtab.device): rtab}

        def fn():
            with hb.deterministic(True):
                feats = fe.run(samples, offsets, fr, max(max(frames), 1))
                res = torch.full((int(ooffs[-1]),), float("nan"), device=DEV)
                hb.resample(plan, samples, offsets, fac, oo, res, max_out=max(olens))
                rev = torch.full((total,), float("nan"), device=DEV)
                hb.reverb(rplan, samples, offsets, rir, rev, max_len=max(c["lens"]))
                mix, gains = torch.full((total,), float("nan"), device=DEV), torch.full((len(rows),), float("nan"), device=DEV)
                hb.noise_mix(bank, samples, offsets, clip, start, scale, out=mix, max_len=max(c["lens"]), gains=gains)
            assert fe.plan.on(feats.device) is fplan and plan.on(res.device) is rtab, "the kernels read another image"
            for t in (feats, res, rev, mix, gains):
                assert bool(torch.isfinite(t).all())
            return dict(feats=feats, resampled=res, reverb=rev, mix=mix, gains=gains)
        return fn, [samples, offsets, fr, fac, oo, rir, clip, start, scale, fplan, rtab]
    _case("Frontend.run, resample, reverb, noise_mix", build)


# ------------------------------------------------------------------------------------------------- one whole step
@pytest.mark.parametrize("det", [False, True])
def test_supervised_train_step(hb, tmp_path, monkeypatch, det):
    """One Solver.sup_train_one_iteration at the tiny shape with ctc_weight 0.3 (test_ctc_gpu's solver and batch), every
    allocation of the step fenced - the arena buffer as a whole, the pooled workspaces, the flat gradient buffer: all bands
    intact, and the loss equals the unguarded step's - bit for bit in deterministic mode, inside test_deterministic_gpu's
    LOSS_GATE (twice, as test_poison_gpu holds two default-path runs to each other) otherwise."""
    import ops
    import test_ctc_gpu as TC
    import test_deterministic_gpu as TD
    losses, total, n_bands = {}, G.Stats(), 0
    for p in (None,) + G.INT_PATTERNS:
        solver, dev = TC._solver(str(tmp_path / str(p)), monkeypatch, ctc_weight=0.3, deterministic=det)
        torch.manual_seed(3)
        np.random.seed(4)
        hb.persist_clear_abort(dev)
        P.empty_pool()
        ops._ARENA.__init__()
        batch = TC._sup_batch(dev)
        st = G.Stats()
        if p is None:
            loss = solver.sup_train_one_iteration(*batch, 1.0)
            solver.flush()
        else:
            with G.guarded(p, st):
                loss = solver.sup_train_one_iteration(*batch, 1.0)
                solver.flush()
        losses[p] = float(loss)
        n_bands += G.check(st)
        assert not hb.persist_aborted(dev)
        P.empty_pool()
        if p is not None:
            assert st.unfenced == [], st.unfenced
            assert st.n_allocs > 0
            st.records = []
            total.merge(st)
    rtol, atol = TD.LOSS_GATE
    for p in G.INT_PATTERNS:
        assert np.isfinite(losses[p])
        if det:
            assert losses[p] == losses[None], "loss %.9g guarded (%s), %.9g unguarded" % (losses[p], p, losses[None])
        else:
            assert abs(losses[p] - losses[None]) <= 2.0 * (rtol * abs(losses[None]) + atol), (p, losses)
    print("guard_coverage %-44s %s; %d bands checked; intact, loss %s; module %.1f s"
          % ("sup train step ctc_weight 0.3 %s" % ("deterministic" if det else "default"), total.line(), n_bands,
             "bit-identical" if det else "inside the gate", time.time() - _T0))

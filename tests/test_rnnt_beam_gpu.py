"""The transducer beam search on the GPU (csrc/rnnt_beam.hip) against tests/rnnt_beam_ref.py.

Every batch is ragged, holds an utterance without a frame where the case has one, and carries NaN in the encoder output (so in
PE) behind every utterance: a frame t >= T_b that is read shows.  The grid is rnnt_beam_ref.GRID (the step kernel has one
shape - 256 threads, K-entry register lists - so the grid straddles what its loops depend on: V and J either side of a
wave's 64 lanes, J past 256, one entry / several / 16, fewer candidates than K, T' = 1, L = 1 and L > T').  Hypotheses and
order are compared where rnnt_beam_ref.judge is decisive; scores within its allowance."""
import numpy as np
import pytest
import torch

import poison as P
import rnnt_beam_ref as BR
import rnnt_ref as R
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


@pytest.fixture(autouse=True)
def _clean_pools():
    yield
    P.empty_pool()


def _head(p):
    import model as M
    V, E = p["embedding.weight"].shape
    J, H = p["lin_enc.weight"].shape
    head = M.TransducerHead(V, E, p["lstm.weight_hh_l0"].shape[1], H, J, bos=1).to(DEV)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return head


def _batch(utts, extra=1):
    """[enc_h [T_b, H]] -> (enc_h [B, max T_b + extra, H] with NaN behind every utterance, lens on the device)."""
    import hip_backend as hb
    T = max(max(u.shape[0] for u in utts), 1) + extra
    x = np.full((len(utts), T, utts[0].shape[1]), np.nan, np.float32)
    for b, u in enumerate(utts):
        x[b, :u.shape[0]] = u
    return torch.from_numpy(x).to(DEV), hb.to_device_i32([u.shape[0] for u in utts], DEV)


def _run(head, utts, K, L, extra=1, **kw):
    x, lens = _batch(utts, extra)
    with torch.no_grad():
        out = head.beam(x, lens, K, L, **kw)
    return [t.cpu().numpy() for t in out]


def _rows(out):
    """-> per utterance [(tokens, score)] of the used slots; checks the layout on the way."""
    hyp, hyp_len, score = out[:3]
    res = []
    for b in range(hyp.shape[0]):
        used = int((hyp_len[b] >= 0).sum())
        assert used >= 1 and (hyp_len[b, :used] >= 0).all() and (hyp_len[b, used:] == -1).all()
        assert np.isfinite(score[b, :used]).all() and np.isneginf(score[b, used:]).all()
        assert (np.diff(score[b, :used]) <= 0).all()
        assert (hyp[b, used:] == -1).all()
        rows = []
        for k in range(used):
            n = int(hyp_len[b, k])
            assert (hyp[b, k, n:] == -1).all()
            rows.append((tuple(int(v) for v in hyp[b, k, :n]), float(score[b, k])))
        assert len(set(r[0] for r in rows)) == len(rows)
        res.append(rows)
    return res


def _loss_bound(head, utts, rows):
    """-ops.rnnt_loss of every returned hypothesis of the utterances with a frame -> {(b, tokens): log P}."""
    keys = [(b, tok) for b, r in enumerate(rows) if utts[b].shape[0] for tok, _ in r]
    x, lens = _batch([utts[b] for b, _ in keys])
    ys = [torch.tensor(tok, dtype=torch.long, device=DEV) for _, tok in keys]
    with torch.no_grad():
        nll = head.nll(x, ys, lens).cpu().numpy()
    return {k: -float(v) for k, v in zip(keys, nll)}


def _compare(what, p, utts, K, L, out, head=None, tot=None, **lm):
    """Well-formed output; the reference's hypotheses, order and scores where judge() is decisive; with `head` the bound
    tot <= -ops.rnnt_loss(hyp) + allowance, the allowance the judge's and nothing else; the excess over the bound is
    printed as a fraction of it."""
    rows = _rows(out)
    V = p["lin_out.weight"].shape[0]
    bound = _loss_bound(head, utts, rows) if head is not None else {}
    worst = 0.0
    for b, enc_h in enumerate(utts):
        assert all(1 <= v < V for tok, _ in rows[b] for v in tok) and all(len(tok) <= L for tok, _ in rows[b])
        if enc_h.shape[0] == 0 and not lm:
            assert rows[b] == [((), 0.0)]
        j = BR.judge(dict(p=p, enc_h=enc_h, bos=1, K=K, L=L, **lm))
        want = j["ref"]["finals"][:K]
        assert len(rows[b]) == len(want), (what, b, rows[b], [f["tokens"] for f in want])
        tots = [s for _, s in rows[b]] if tot is None else [float(v) for v in tot[b, :len(rows[b])]]
        over = [(t - bound[(b, tok)]) / j["allowance"] for (tok, _), t in zip(rows[b], tots) if (b, tok) in bound]
        if over:
            print("rnnt-beam-bound %s row %d: tot - log P at most %.3f of the allowance %.3g" % (what, b, max(over), j["allowance"]))
            assert max(over) <= 1.0, (what, b, max(over))
        if not j["decisive"]:
            print("rnnt-beam-parity %s row %d: undecided" % (what, b))
            continue
        assert [tok for tok, _ in rows[b]] == [f["tokens"] for f in want], (what, b)
        allow = max(j["allowance"], 8 * ULP)
        err = max(abs(s - float(f["rank"])) for (_, s), f in zip(rows[b], want))
        err = max([err] + [abs(t - float(f["tot"])) for t, f in zip(tots, want)])
        print("rnnt-beam-parity %s row %d: err %.3g, allowance %.3g, ratio %.3f" % (what, b, err, allow, err / allow))
        worst = max(worst, err / allow)
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("V,K,J,lens,L,seed", BR.GRID, ids=["V%d-K%d-J%d-T%d-L%d" % (g[0], g[1], g[2], max(g[3]), g[4]) for g in BR.GRID])
def test_grid(hb, V, K, J, lens, L, seed):
    p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
    head = _head(p)
    out = _run(head, utts, K, L)
    _compare("grid V%d K%d J%d T%d L%d" % (V, K, J, max(lens), L), p, utts, K, L, out, head=head)


def test_exhaustive(hb):
    """V = 3, L = 3, K = 16: all 15 sequences, each within the allowance of -ops.rnnt_loss from both sides."""
    p, _ = BR.grid_case(3, 8, 1, 31)
    utts = [BR.grid_case(3, 8, T, 31)[1] for T in (1, 2, 4)]
    head = _head(p)
    out = _run(head, utts, 16, 3)
    rows = _rows(out)
    _compare("exhaustive", p, utts, 16, 3, out, head=head)
    bound = _loss_bound(head, utts, rows)
    for b, r in enumerate(rows):
        assert len(r) == 15
        allow = BR.judge(dict(p=p, enc_h=utts[b], bos=1, K=16, L=3))["allowance"]
        worst = max(abs(s - bound[(b, tok)]) for tok, s in r) / allow
        print("rnnt-beam-exhaustive row %d: |tot - log P| at most %.3f of the allowance %.3g" % (b, worst, allow))
        assert worst <= 1.0, (b, worst)


@pytest.mark.parametrize("K", (1, 2, 4, 16))
def test_tie_rule(hb, K):
    """lin_out zero, one frame: every candidate of one length ties and nothing merges - the order is the rule's."""
    p = BR.tie_params(3, 4, 3)
    utts = [np.ones((1, 16), np.float32), np.zeros((0, 16), np.float32), -np.ones((1, 16), np.float32)]
    rows = _rows(_run(_head(p), utts, K, 3))
    for b, enc_h in enumerate(utts):
        want = BR.search(p, enc_h, 1, K, 3)["finals"][:K]
        assert [tok for tok, _ in rows[b]] == [f["tokens"] for f in want], (K, b, rows[b])


@pytest.mark.parametrize("K", (1, 2, 4, 16))
def test_tie_rule_blank_against_labels(hb, K):
    """lin_out zero, two frames, L = 1: at iteration 0 the blank (flat index 0) ties with both labels inside one selection
    and wins; at iteration 1 the two merged candidates tie and keep their slot order.  Every tie here is between values
    formed by the same operations (the same bits whatever a last-bit rounding does); the classes are log 2 or more apart."""
    p = BR.tie_params(3, 4, 3)
    utts = [np.ones((2, 16), np.float32), np.zeros((0, 16), np.float32), -np.ones((2, 16), np.float32)]
    rows = _rows(_run(_head(p), utts, K, 1))
    want = {1: [()], 2: [(), (1,)]}.get(K, [(), (1,), (2,)])
    for b, enc_h in enumerate(utts):
        ref = [f["tokens"] for f in BR.search(p, enc_h, 1, K, 1)["finals"][:K]]
        assert [tok for tok, _ in rows[b]] == ref and (enc_h.shape[0] == 0 or ref == want), (K, b, rows[b], ref)


@pytest.mark.parametrize("name", sorted(R.DECODE_CASES))
def test_beam_one_against_greedy(hb, name):
    """K = 1 returns greedy's tokens (max_symbols = L) on the rows where the float64 restatement's best final is greedy's
    hypothesis and judge() is decisive (test_rnnt_beam_cpu.py holds that each case has such a row)."""
    p, enc_h, lens, _, max_len = R.decode_case(name)
    head = _head(p)
    utts = [enc_h[b, :t] for b, t in enumerate(lens)]
    rows = _rows(_run(head, utts, 1, max_len))
    x, ld = _batch(utts, 0)
    with torch.no_grad():
        out, n, _ = head.greedy(x, ld, max_len, max_len)
    out, n = out.cpu().numpy(), n.cpu().numpy()
    checked = 0
    for b, u in enumerate(utts):
        greedy = tuple(int(v) for v in out[b, :n[b]])
        j = BR.judge(dict(p=p, enc_h=u, bos=1, K=1, L=max_len))
        if j["decisive"] and j["ref"]["finals"][0]["tokens"] == tuple(R.greedy(p, u, 1, max_len, max_len)["tokens"]):
            assert rows[b][0][0] == greedy, (name, b)
            checked += 1
    assert checked >= 1


def _bits(out):
    return [t.tobytes() for t in out]


def test_reproducible_and_independent(hb):
    V, K, J, lens, L, seed = BR.GRID[5]
    p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
    head = _head(p)
    first = _run(head, utts, K, L)
    assert _bits(first) == _bits(_run(head, utts, K, L))
    with hb.deterministic():
        assert _bits(first) == _bits(_run(head, utts, K, L))
    for b, u in enumerate(utts):                                     # a row alone: the bits it has inside the batch
        alone = _run(head, [u], K, L)
        for a, f in zip(alone, first):
            assert a[0].tobytes() == f[b].tobytes(), b


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_poisoned_buffers(hb, pattern):
    """From an empty pool and from the poisoned leftover of a larger call in the same capacity class: the clean bits, with
    and without the LM.  The workspace holds integer regions (slot, token, state, counters): every one of them is written by
    the init kernel or the step kernel before a kernel of the call reads it, and what indexes memory is clamped."""
    import ops
    V, K, J, lens, L, seed = BR.GRID[3]
    p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
    head = _head(p)
    lm = dict(ngram=_lm(V), ngram_weight=0.7, ngram_bonus=0.3)
    P.empty_pool()
    clean = _bits(_run(head, utts, K, L)) + _bits(_run(head, utts, K, L, **lm))
    for variant in ("empty pool", "leftover"):
        P.empty_pool()
        st = P.Stats()
        if variant == "leftover":
            _run(head, utts, K, L + 2)
            keys = [k for k in ops._POOL.free if k[0] == "rnnt_beam"]
            assert len(keys) == 1 and P.poison_pool(pattern, st) >= 1
        with P.poisoned(pattern, st):
            got = _bits(_run(head, utts, K, L)) + _bits(_run(head, utts, K, L, **lm))
        if variant == "leftover":
            assert [k for k in ops._POOL.free if k[0] == "rnnt_beam"] == keys      # (the same capacity class: the leftover was used)
        assert st.total > 0 and got == clean, (pattern, variant)
        print("rnnt-beam-poison %-5s %-10s %s; bit-identical" % (pattern, variant, st.line()))


_LMS = {}


def _lm(V):
    if V not in _LMS:
        import ngram
        rs = np.random.RandomState(V)
        seqs = [[int(t) for t in rs.randint(3, V, rs.randint(1, 6))] for _ in range(40)]
        _LMS[V] = ngram.NgramLM.estimate(seqs, 3, V, 1, 2)
    return _LMS[V]


@pytest.mark.parametrize("eos_term", (True, False))
def test_ngram(hb, eos_term):
    import ops
    V, K, J, lens, L, seed = BR.GRID[5]
    p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
    head = _head(p)
    lm = _lm(V)
    plain = _run(head, utts, K, L)
    zero = _run(head, utts, K, L, ngram=lm, eos_term=eos_term)
    assert _bits(plain) == _bits(zero[:3]) and zero[3].tobytes() == plain[2].tobytes()
    out = _run(head, utts, K, L, ngram=lm, ngram_weight=0.7, ngram_bonus=0.3, eos_term=eos_term)
    _compare("ngram eos %d" % eos_term, p, utts, K, L, out, head=head, tot=out[3], table=lm.compile(), alpha=0.7, beta=0.3,
             eos_term=eos_term)
    hyp, hyp_len, score, tot, lms = out
    want = ops.ngram_score(lm, torch.from_numpy(hyp.reshape(-1, L)).to(DEV).clamp(min=0),
                           torch.from_numpy(hyp_len.reshape(-1)).to(DEV), eos_term=eos_term).cpu().numpy().reshape(lms.shape)
    used = hyp_len >= 0
    assert np.isneginf(lms[~used]).all() and np.isneginf(tot[~used]).all()
    assert np.abs(lms[used] - want[used]).max() <= 8 * ULP * max(1.0, np.abs(want[used]).max())
    f32 = np.float32
    assert np.array_equal(score[used], (tot[used] + f32(0.7) * lms[used]) + f32(0.3) * hyp_len[used].astype(f32))


def test_launches_per_iteration(hb):
    """Four launches per iteration (step kernel, gate product, cell kernel, projection; the last iteration is the step
    kernel alone), four before the loop (init, gate product, cell, projection), one behind it: 4 (T' + L) + 2."""
    V, K, J, lens, L, seed = BR.GRID[2]
    p, utts = BR.grid_utterances(V, K, J, lens, L, seed)
    head = _head(p)
    x, ld = _batch(utts)
    with torch.no_grad():
        pe = head.project_enc(x)
        before = dict(hb.LAUNCHES)
        w_ih, w_hh, b_ih, b_hh = head.lstm.direction_params(0)
        import ops
        ops.rnnt_beam(pe, ld, torch.cat([w_ih, w_hh], 1).contiguous(), (b_ih + b_hh).contiguous(), head.lin_pred.weight,
                      head.lin_out.weight, head.lin_out.bias, head.embedding.weight, 1, K, L)
    T = x.shape[1]
    # the counter adds one per product: each of the two products IS one kernel (no zero pass, no pass behind)
    rows, E, P = len(utts) * K, head.embedding.weight.shape[1], head.pred_dim
    for plan in (hb.gemm_plan(rows, 4 * P, E + P, trans_b=True, bias=True, split_k=1),
                 hb.gemm_plan(rows, J, P, trans_b=True, split_k=1)):
        assert plan["rc"] == 0 and len(plan["launches"]) == 1, plan["launches"]
    assert hb.LAUNCHES["rnnt_beam_launch"] - before.get("rnnt_beam_launch", 0) == 4 * (T + L) + 2
    assert hb.LAUNCHES["rnnt_beam_step"] - before.get("rnnt_beam_step", 0) == T + L


def test_refusals(hb):
    p, utts = BR.grid_utterances(*BR.GRID[2])
    head = _head(p)
    for K in (0, 17):
        with pytest.raises(hb.UnsupportedShape):
            _run(head, utts, K, 4)
    with pytest.raises(ValueError):
        _run(head, utts, 2, 0)
    with pytest.raises(hb.UnsupportedShape):
        hb.rnnt_beam_ws_bytes(3, 8, 30, 34, 4, 4, 16, 16)              # J % 4
    with pytest.raises(hb.UnsupportedShape):
        hb.rnnt_beam_ws_bytes(3, 8, 1024, 34, 16, 4, 16, 16)           # 16 (1024 + 34) floats of LDS
    assert hb.rnnt_beam_ws_bytes(3, 8, 260, 65, 16, 40, 16, 16) > 0
    with pytest.raises(hb.UnsupportedShape):
        _run(head, utts, 2, 4, ngram=_lm(34))                        # an LM over another vocabulary


# ------------------------------------------------------------------------------------------------ model and solver
def _tiny(**kw):
    import model as M
    torch.manual_seed(21)
    net = M.E2E(labeldist=synth.labeldist(synth.TINY["output_dim"], 12), **synth.TINY, **kw).to(DEV)
    weights = {k: torch.from_numpy(v) for k, v in synth.e2e_weights(synth.TINY, 11).items()}
    net.load_state_dict(weights, strict=False)
    net.eval()
    xs, ilens, _ = synth.batch(synth.TINY["input_dim"], synth.TINY["output_dim"], synth.TINY_ILENS, synth.TINY_YLENS, 13)
    return net, torch.from_numpy(xs).to(DEV), ilens


def test_recognize_rnnt_beams(hb):
    """E2E.recognize_rnnt_beams against the float64 search of the head's weights on the model's own encoder output."""
    net, xs, ilens = _tiny(rnnt_weight=0.3, rnnt_joint_dim=32)
    K, L = 4, 6
    ids = net.recognize_rnnt_beams(xs, ilens, K, max_dec_timesteps=L)
    last = net.last_rnnt_beams
    assert tuple(last["tokens"].shape) == (len(ilens), K, L) and last["parts"] == {}
    with torch.no_grad():
        enc_h, _ = net.encoder(xs, ilens)
    frames = net.encoder.enc2.last_lens_dev.cpu().tolist()
    p = {k: v.detach().cpu().numpy() for k, v in net.rnnt.state_dict().items()}
    utts = [enc_h[b, :frames[b]].cpu().numpy() for b in range(len(ilens))]
    out = [last[k].cpu().numpy() for k in ("tokens", "lengths", "scores")]
    _compare("model", p, utts, K, L, out)
    assert ids == [list(r[0][0]) for r in _rows(out)]
    net.recognize_rnnt_beams(xs, ilens, 2, max_dec_timesteps=L, ngram=_lm(synth.TINY["output_dim"]), ngram_weight=0.5)
    assert set(net.last_rnnt_beams["parts"]) == {"rnnt", "lm"}
    # K = 1 against E2E.recognize_rnnt(max_symbols = L), on the rows where the float64 search's best final is greedy's
    one = net.recognize_rnnt_beams(xs, ilens, 1, max_dec_timesteps=L)
    greedy = net.recognize_rnnt(xs, ilens, max_symbols=L, max_dec_timesteps=L)
    checked = 0
    for b, u in enumerate(utts):
        j = BR.judge(dict(p=p, enc_h=u, bos=1, K=1, L=L))
        if j["decisive"] and j["ref"]["finals"][0]["tokens"] == tuple(R.greedy(p, u, 1, L, L)["tokens"]):
            assert one[b] == greedy[b], b
            checked += 1
    print("rnnt-beam K = 1 against recognize_rnnt: %d of %d rows compared" % (checked, len(utts)))
    assert checked >= 1
    plain = _tiny()[0]
    with pytest.raises(ValueError, match="needs the transducer head"):
        plain.recognize_rnnt_beams(xs, ilens, 2)


def test_solver(hb, tmp_path, monkeypatch, capsys):
    """Solver.test with rnnt_beam_decode runs and reports the best-of-K CER; the refusals; a configuration without the key
    launches what rnnt_greedy_decode launched before."""
    import test_ctc_gpu as TC
    solver, dev = TC._solver(str(tmp_path / "s"), monkeypatch, rnnt_weight=0.3, rnnt_joint_dim=32)
    state = {k: v.clone() for k, v in solver.model.state_dict().items()}
    solver.config.update(rnnt_greedy_decode=True)
    before = dict(hb.LAUNCHES)
    solver.test(state_dict=state)
    greedy = {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}
    assert greedy.get("rnnt_greedy_step", 0) > 0 and not any(k.startswith("rnnt_beam") for k in greedy)
    solver.config.update(rnnt_beam_decode=False)                     # the key present and off: launch for launch the same
    before = dict(hb.LAUNCHES)
    solver.test(state_dict=state)
    assert {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)} == greedy
    solver.config.update(rnnt_greedy_decode=False, rnnt_beam_decode=True, beam_size=4, cer_on_gpu=True, max_dec_timesteps=12)
    capsys.readouterr()
    cer = solver.test(state_dict=state)
    text = capsys.readouterr().out
    assert np.isfinite(cer) and "best of 4 hypotheses: CER=" in text
    assert solver.last_test["best_of_k_cer"] <= cer and len(solver.last_test["dist"][0]) == 4
    for extra, msg in ((dict(rnnt_greedy_decode=True), "does not combine with rnnt_greedy_decode"),
                       (dict(ctc_greedy_decode=True), "ctc_greedy_decode decodes with the CTC head alone"),   # (the older refusal)
                       (dict(ctc_beam_decode=True), "does not combine with ctc_beam_decode"),
                       (dict(two_pass_decode=True), "does not combine with two_pass_decode"),
                       (dict(word_lm="x.arpa"), "does not combine with word_lm"),
                       (dict(lm_weight=0.3), "does not combine with lm_weight > 0"),
                       (dict(ctc_decode_weight=0.3), "does not combine with ctc_decode_weight > 0"),
                       (dict(ngram_weight=0.3), "ngram_weight is set without ngram_lm")):
        solver.config.update(extra)
        with pytest.raises(ValueError, match=msg):
            solver.test(state_dict=state)
        for k in extra:
            del solver.config[k]
    # with ngram_lm: the ARPA file is read, the LM sits inside the search (the n-best carries its parts)
    import ngram
    nv = len(solver.vocab)
    rs = np.random.RandomState(7)
    lm = ngram.NgramLM.estimate([[int(t) for t in rs.randint(3, nv, rs.randint(1, 6))] for _ in range(30)], 2, nv,
                                solver.vocab["<BOS>"], solver.vocab["<EOS>"])
    arpa = tmp_path / "lm.arpa"
    arpa.write_text(lm.to_arpa({i: s for s, i in solver.vocab.items()}))
    solver.config.update(ngram_lm=str(arpa), ngram_weight=0.5, ngram_bonus=0.2)
    plain_scores = solver.model.last_rnnt_beams["scores"].clone()
    cer = solver.test(state_dict=state)
    last = solver.model.last_rnnt_beams
    assert np.isfinite(cer) and set(last["parts"]) == {"rnnt", "lm"} and not torch.equal(last["scores"], plain_scores)
    used = last["lengths"] >= 0
    want = (last["parts"]["rnnt"][used] + last["parts"]["lm"][used] * 0.5) + last["lengths"][used].float() * 0.2
    assert torch.equal(last["scores"][used], want)
    for k in ("ngram_lm", "ngram_weight", "ngram_bonus"):
        del solver.config[k]
    headless, _ = TC._solver(str(tmp_path / "h"), monkeypatch)
    headless.config.update(rnnt_beam_decode=True)
    with pytest.raises(ValueError, match="rnnt_beam_decode needs the transducer head"):
        headless.test(state_dict=headless.model.state_dict())

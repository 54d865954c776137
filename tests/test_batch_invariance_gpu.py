"""No sequence kernel's result may depend on the rest of the batch.  Every loss, alignment, search and front-end kernel takes
a row index, a frame length from the device, a row stride, a time extent no row may fill and often a packed side table; an
utterance's outputs are a function of that utterance alone.  Each test here runs one case table of tests/batch_cases.py four
ways (batch_cases.arrangements):

  base     the utterances in their order, T = the longest, ld = V
  alone    every utterance as a batch of one, T = max(T_b, 1), the packed side inputs at offset 0
  moved    the order reversed behind one extra, strictly longer utterance (batch_cases.moved_order: no utterance keeps its
           row): every row index, packed offset and the extent change; the context graphs in another order than the rows
  padded   the base order on T + 5 frames and ld = V + 3, NaN behind every length and in the padding columns

and asserts that every output an utterance owns (its slice [:T_b], its packed label range) has in the three transformed runs
the BITS it has in the base run, and that every run carries the documented filler outside the slice (-1, -inf, 0, zero
gradient).  No tolerance: no output took the allowance exit.  Each test prints one `batch-invariance` line per kernel and
transformation - rows compared, then words compared / words different per output (`pytest -s`;
profiles/batch_invariance.txt holds one run)."""
import numpy as np
import pytest
import torch

import batch_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _words(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.int32, np.int64), a.dtype
    return a.reshape(-1).view(np.int32)


def _invariance(kernel, utts, extra, run):
    """run(rows, name, extra_frames, extra_cols) -> one dict per row {output: the array that row owns}; the run itself
    asserts the filler.  Compares every transformed run with the base run, prints the record, asserts no word differs."""
    base, stats = None, {}
    for name, rows, owner, ef, ec in B.arrangements(utts, extra):
        got = run(rows, name, ef, ec)
        assert len(got) == len(rows)
        if name == "base":
            base = got
            continue
        for r, b in enumerate(owner):
            if b == B.EXTRA:
                continue
            assert sorted(got[r]) == sorted(base[b])
            for out, a in got[r].items():
                x, y = _words(a), _words(base[b][out])
                assert x.shape == y.shape, (kernel, name, out, b)
                s = stats.setdefault(name, {}).setdefault(out, [0, 0, 0])
                s[0], s[1], s[2] = s[0] + 1, s[1] + x.size, s[2] + int((x != y).sum())
    bad = []
    for name in ("alone", "moved", "padded"):
        outs = stats[name]
        assert sorted(outs) == sorted(base[0]), "an output was left out of %s" % name
        assert all(s[0] == len(utts) and s[1] > 0 for s in outs.values()), "a row or an output was skipped: %r" % outs
        print("batch-invariance %-26s %-6s rows %d  %s" % (kernel, name, len(utts), "  ".join(
            "%s %d/%d" % (o, outs[o][1], outs[o][2]) for o in sorted(outs))))
        bad += ["%s %s %s: %d of %d words" % (kernel, name, o, s[2], s[1]) for o, s in outs.items() if s[2]]
    assert not bad, "an utterance's output depends on the rest of the batch: " + "; ".join(bad)


def _i32(hb, values):
    return hb.to_device_i32([int(v) for v in values], DEV)


def _det(hb, det):
    return hb.deterministic(det)


# ------------------------------------------------------------------------------------------------- 1: the CTC loss
@pytest.mark.parametrize("det", [False, True])
def test_ctc_loss(hb, det):
    """nll[b] and dlogits[b, :T_b]; a zero gradient behind every length and in the padding columns; the infeasible row has
    loss 0 and a zero gradient in every run.  One row on each of the wave, block and strided paths in the same batch."""
    import ops
    utts, extra = B.ctc_utts()

    def run(rows, name, ef, ec):
        c = B.frames_batch(rows, ef, ec)
        V = c["V"]
        buf = torch.from_numpy(c["buf"]).to(DEV).requires_grad_()
        nll = ops.ctc_loss(buf[:, :, :V], _i32(hb, c["lens"]), torch.from_numpy(c["labels"]).to(DEV), c["label_lens"])
        nll.backward(torch.from_numpy(c["g"]).to(DEV))
        nll, grad = nll.detach().cpu().numpy(), buf.grad.cpu().numpy()
        assert grad.shape == c["buf"].shape and not grad[:, :, V:].any()
        out = []
        for i, (u, t) in enumerate(zip(rows, c["lens"])):
            assert not grad[i, t:].any(), "%s: row %d has a gradient behind its %d frames" % (name, i, t)
            if u is utts[B.CTC_INFEASIBLE]:
                assert nll[i] == 0.0 and not grad[i].any()
            else:
                assert np.isfinite(nll[i]) and np.isfinite(grad[i]).all()
            out.append(dict(nll=nll[i:i + 1], dlogits=grad[i, :t, :V]))
        return out

    with _det(hb, det):
        _invariance("ctc_loss det=%d" % det, utts, extra, run)


# ------------------------------------------------------------------------------------------------- 2: the transducer
@pytest.mark.parametrize("det", [False, True])
def test_rnnt_loss(hb, det):
    """nll[b] and dlogits[b, :T_b, :U_b + 1]; the alone run has U + 1 = U_b + 1 label positions, so the position stride
    changes as well.  A zero gradient on every padded node and column."""
    import ops
    utts, extra = B.rnnt_utts()

    def run(rows, name, ef, ec):
        c = B.rnnt_batch(rows, ef, ec)
        V = c["V"]
        buf = torch.from_numpy(c["buf"]).to(DEV).requires_grad_()
        labels = torch.from_numpy(c["labels"]).to(DEV)
        nll = ops.rnnt_loss(buf[..., :V], _i32(hb, c["lens"]), labels, c["label_lens"])
        nll.backward(torch.from_numpy(c["g"]).to(DEV))
        nll, grad = nll.detach().cpu().numpy(), buf.grad.cpu().numpy()
        assert np.isfinite(nll).all() and not grad[..., V:].any()
        out = []
        for i, (t, u) in enumerate(zip(c["lens"], c["label_lens"])):
            assert not grad[i, t:].any() and not grad[i, :, u + 1:].any()
            out.append(dict(nll=nll[i:i + 1], dlogits=grad[i, :t, :u + 1, :V]))
        return out

    with _det(hb, det):
        _invariance("rnnt_loss det=%d" % det, utts, extra, run)


@pytest.mark.parametrize("det", [False, True])
def test_rnnt_joint(hb, det):
    """Z[b, :T_b, :U_b + 1], dpe[b, :T_b], dpp[b, :U_b + 1]; exact zeros on every padded node of Z, dpe and dpp.  The
    operands are contiguous by the operator's contract: the padded run adds the five frames, not columns."""
    import ops
    utts, extra = B.rnnt_utts()

    def run(rows, name, ef, ec):
        c = B.joint_batch(rows, ef)
        pe, pp = (torch.from_numpy(c[k]).to(DEV).requires_grad_() for k in ("pe", "pp"))
        z = ops.rnnt_joint(pe, pp, _i32(hb, c["lens"]), c["label_lens"])
        got_z = z.detach().cpu().numpy().copy()
        z.backward(torch.from_numpy(c["dz"]).to(DEV))
        dpe, dpp = pe.grad.cpu().numpy(), pp.grad.cpu().numpy()
        out = []
        for i, (t, u) in enumerate(zip(c["lens"], c["label_lens"])):
            assert not got_z[i, t:].any() and not got_z[i, :, u + 1:].any() and not dpe[i, t:].any() and not dpp[i, u + 1:].any()
            out.append(dict(z=got_z[i, :t, :u + 1], dpe=dpe[i, :t], dpp=dpp[i, :u + 1]))
        return out

    with _det(hb, det):
        _invariance("rnnt_joint det=%d" % det, utts, extra, run)


# ------------------------------------------------------------------------------------------------- 3: alignment, best path
def test_ctc_align(hb):
    """path[b, :T_b], the score and the packed first / last / token_logp of the utterance's label range; -1 behind every
    length; the two rows that cannot be aligned are -1 / -inf throughout in every run."""
    import ops
    utts, extra = B.align_utts()

    def run(rows, name, ef, ec):
        c = B.frames_batch(rows, ef, ec)
        res = ops.ctc_align(torch.from_numpy(c["buf"]).to(DEV)[:, :, :c["V"]], _i32(hb, c["lens"]),
                            torch.from_numpy(c["labels"]).to(DEV), c["label_lens"])
        path, score = res.path.cpu().numpy(), res.score.cpu().numpy()
        first, last, tlp = res.first.cpu().numpy(), res.last.cpu().numpy(), res.token_logp.cpu().numpy()
        assert res.offsets.cpu().tolist() == c["offsets"].tolist()
        out = []
        for i, (u, t) in enumerate(zip(rows, c["lens"])):
            sl = slice(int(c["offsets"][i]), int(c["offsets"][i + 1]))
            assert (path[i, t:] == -1).all()
            if u is utts[-1]:
                assert np.isneginf(score[i]) and (path[i] == -1).all() and (first[sl] == -1).all() and (last[sl] == -1).all()
                assert np.isneginf(tlp[sl]).all()
            else:
                assert np.isfinite(score[i]) and (path[i, :t] >= 0).all() and np.isfinite(tlp[sl]).all()
            # (an utterance without labels owns an empty packed range: its length is compared through `n_labels`)
            out.append(dict(path=path[i, :t], score=score[i:i + 1], first=first[sl], last=last[sl], token_logp=tlp[sl],
                            n_labels=np.array([sl.stop - sl.start], dtype=np.int32)))
        return out

    with _det(hb, True):
        _invariance("ctc_align", utts, extra, run)


def test_ctc_greedy(hb):
    """ids[b, :n_b], n[b], frame_tok[b, :T_b]; -1 behind the hypothesis and behind every length."""
    import ops
    utts, extra = B.align_utts()

    def run(rows, name, ef, ec):
        c = B.frames_batch(rows, ef, ec)
        ids, n, frame_tok = (x.cpu().numpy() for x in ops.ctc_greedy(torch.from_numpy(c["buf"]).to(DEV)[:, :, :c["V"]],
                                                                     _i32(hb, c["lens"])))
        out = []
        for i, t in enumerate(c["lens"]):
            assert 0 <= n[i] <= t and (ids[i, n[i]:] == -1).all() and (frame_tok[i, t:] == -1).all()
            assert (ids[i, :n[i]] > 0).all() and (frame_tok[i, :t] >= 0).all()
            out.append(dict(ids=ids[i, :t], n=n[i:i + 1], frame_tok=frame_tok[i, :t]))
        return out

    with _det(hb, True):
        _invariance("ctc_greedy", utts, extra, run)


# ------------------------------------------------------------------------------------------------- 4: the CTC beam search
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", sorted(B.BEAM))
@pytest.mark.parametrize("mode", B.MODES)
def test_ctc_beam(hb, mode, name, det):
    """Every returned tensor of every mode: hyp[b, :, :T_b], hyp_len, score, ctc_score, lm_score, n_words, ctx_score.  Unused
    slots hold -1 / -inf behind every used one, hyp is -1 behind each hypothesis.  Batch (b): row 0 writes its history to
    the workspace; row 1 stays in LDS beside it, stays in LDS without a workspace region when alone, and in the moved run
    both sit behind a longer row, at other row indices and on another extent T."""
    import ops
    utts, extra, fixtures = B.beam_utts(name)
    K, names = B.BEAM[name]["K"], B.MODE_OUTPUTS[mode]

    def run(rows, arrangement, ef, ec):
        c = B.frames_batch(rows, ef, ec)
        res = ops.ctc_beam(torch.from_numpy(c["buf"]).to(DEV)[:, :, :c["V"]], _i32(hb, c["lens"]), K,
                           **B.beam_kwargs(mode, fixtures, rows, arrangement))
        assert len(res) == len(names)
        got = {k: v.cpu().numpy() for k, v in zip(names, res)}
        assert got["hyp"].shape == (len(rows), K, c["T"])
        out = []
        for i, t in enumerate(c["lens"]):
            used = got["hyp_len"][i] >= 0
            assert used[0] or mode == "word_lm_lexicon"
            assert not used[int(used.sum()):].any() and (got["hyp_len"][i][~used] == -1).all()
            for k in range(K):
                n = max(int(got["hyp_len"][i, k]), 0)
                assert n <= t and (got["hyp"][i, k, n:] == -1).all() and (got["hyp"][i, k, :n] > 0).all()
            for q in names[2:]:
                if q == "n_words":
                    assert (got[q][i][~used] == -1).all() and (got[q][i][used] >= 0).all()
                else:
                    assert np.isneginf(got[q][i][~used]).all() and np.isfinite(got[q][i][used]).all(), (q, i)
            if mode.startswith("context") and rows[i]["graph"] < 0:
                assert (got["ctx_score"][i][used] == 0).all()
            row = {q: got[q][i] for q in names[1:]}
            row["hyp"] = got["hyp"][i, :, :t]
            out.append(row)
        return out

    with _det(hb, det):
        _invariance("ctc_beam %s (%s) det=%d" % (mode, name, det), utts, extra, run)


# ------------------------------------------------------------------------------------------------- 5: MWER
def test_mwer(hb):
    """Per utterance seq_logp, post, coef (its K rows), risk and the dlogits rows of its hypotheses [:L_b]; exact zeros in
    unused slots and behind every hypothesis.  `scale` and the upstream gradient are arguments of the call and the same in
    every run; the summed `loss` is not a per-utterance output and is left out."""
    utts, extra = B.mwer_utts()
    f32 = dict(device=DEV, dtype=torch.float32)

    def run(rows, name, ef, ec):
        c = B.mwer_batch(rows, ef, ec)
        nB, K, L, V = c["B"], c["K"], c["L"], c["V"]
        R = nB * K
        logits = torch.from_numpy(c["buf"]).to(DEV)[:, :, :V]
        tokens, npos, err = (torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "npos", "err"))
        o = {k: torch.full((R,), float("nan"), **f32) for k in ("seq_logp", "post", "coef")}
        risk, loss = torch.full((nB,), float("nan"), **f32), torch.full((1,), float("nan"), **f32)
        ws = torch.full((L * R,), float("nan"), **f32)
        hb.mwer_fwd(logits, tokens, npos, err, nB, B.MWER_SCALE, o["seq_logp"], o["post"], o["coef"], risk, loss, ws)
        dz = torch.full((L, R, V), float("nan"), **f32)
        hb.mwer_bwd(logits, tokens, npos, o["coef"], nB, torch.tensor([B.MWER_G], **f32), B.MWER_SCALE, dz)
        o = {k: v.cpu().numpy() for k, v in o.items()}
        risk, dz = risk.cpu().numpy(), dz.cpu().numpy()
        n = np.clip(c["npos"], 0, L)
        assert not dz.view(np.uint32)[np.arange(L)[:, None] >= n[None, :]].any(), "a masked position of dlogits is not +0.0"
        for k in o:
            assert not o[k].view(np.uint32)[c["npos"] <= 0].any() and np.isfinite(o[k]).all()
        out = []
        for i, u in enumerate(rows):
            Lb, sl = u["logits"].shape[0], slice(i * K, (i + 1) * K)
            row = {k: o[k][sl] for k in o}
            row.update(risk=risk[i:i + 1], dlogits=dz[:Lb, sl])
            assert np.isfinite(row["dlogits"]).all() and np.isfinite(risk[i])
            out.append(row)
        return out

    with _det(hb, True):
        _invariance("mwer", utts, extra, run)


# ------------------------------------------------------------------------------------------------- 6: edit distances
@pytest.mark.parametrize("words", [False, True], ids=["edit_distance", "word_edit_distance"])
def test_edit_distance(hb, words):
    """dist, hyp_n, ref_n of every pair: integers, equal.  The moved run keeps the references in the base order (the extra
    one last) and scores through a ref_index that is no identity; the padded run widens the references by three columns of
    ids no string uses (the hypotheses are at ED_MAX_COLS already: a wider row is refused)."""
    pairs, extra = B.edit_pairs(hb.ED_MAX_COLS)
    assert max(len(p["hyp"]) for p in pairs) == hb.ED_MAX_COLS and len(pairs) == 8

    def run(rows, name, ef, ec):
        order = B.moved_ref_order(len(rows) - 1) if name == "moved" else None
        c = B.pairs_batch(rows, ec, order)
        hyp = torch.from_numpy(c["hyp"][:, :hb.ED_MAX_COLS].copy()).to(DEV)
        ref, ref_len, hyp_len = (torch.from_numpy(c[k]).to(DEV) for k in ("ref", "ref_len", "hyp_len"))
        idx = None if c["ref_index"] is None else torch.from_numpy(c["ref_index"]).to(DEV)
        assert (name == "moved") == (idx is not None) and (idx is None or (c["ref_index"] != np.arange(len(rows))).any())
        if words:
            res = hb.word_edit_distance(hyp, ref, ref_len, B.ED_SPACE, hyp_len=hyp_len, ref_index=idx)
        else:
            res = hb.edit_distance(hyp, ref, ref_len, hyp_len=hyp_len, ref_index=idx)
        dist, hyp_n, ref_n = (x.cpu().numpy() for x in res)
        if not words:
            assert hyp_n.tolist() == [len(p["hyp"]) for p in rows] and ref_n.tolist() == [len(p["ref"]) for p in rows]
        assert (dist >= 0).all()
        return [dict(dist=dist[i:i + 1], hyp_n=hyp_n[i:i + 1], ref_n=ref_n[i:i + 1]) for i in range(len(rows))]

    with _det(hb, True):
        _invariance("word_edit_distance" if words else "edit_distance", pairs, extra, run)


# ------------------------------------------------------------------------------------------------- 7: the packed front end
def _packed(hb, rows, tail):
    c = B.waves_batch(rows, tail)
    return c, torch.from_numpy(c["samples"]).to(DEV), torch.from_numpy(c["offsets"]).to(DEV)


def test_frontend_features(hb):
    """hb.fbank, the CMVN statistics and feat_finish (deltas of order 2, per-utterance CMVN) as Frontend.run chains them:
    the feature frames [b, :T_b]; zeros behind every utterance.  The 1-sample waveform has no frame: it is compared through
    its frame count."""
    from frontend import Frontend
    rows_, extra, _ = B.waves()
    fe = Frontend(dict(B.FE_CFG))

    def run(rows, name, ef, ec):
        c, samples, offsets = _packed(hb, rows, ef)
        frames = [fe.num_frames(n) for n in c["lens"]]
        t_max = max(max(frames), 1) + ef
        xs = fe.run(samples, offsets, _i32(hb, frames), t_max).cpu().numpy()
        assert xs.shape == (len(rows), t_max, fe.output_dim)
        out = []
        for i, t in enumerate(frames):
            assert not xs[i, t:].any() and np.isfinite(xs[i, :t]).all()
            out.append(dict(feats=xs[i, :t], n_frames=np.array([t], dtype=np.int32)))
        return out

    assert [fe.num_frames(w["x"].size) for w in rows_] == [0, 1, 5]
    with _det(hb, True):
        _invariance("fbank+cmvn+deltas", rows_, extra, run)


def test_resample(hb):
    """The resampled samples of every row, factor_index travelling with the utterance; nothing behind the last offset is
    written."""
    rows_, extra, _ = B.waves()
    plan = hb.ResamplePlan(16000, B.SPEEDS)

    def run(rows, name, ef, ec):
        c, samples, offsets = _packed(hb, rows, ef)
        lens = [plan.out_samples(n, w["factor"]) for n, w in zip(c["lens"], rows)]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        out = torch.full((int(offs[-1]) + ef,), float("nan"), device=DEV)
        hb.resample(plan, samples, offsets, _i32(hb, [w["factor"] for w in rows]), torch.from_numpy(offs).to(DEV), out,
                    max_out=max(lens) + ef)
        out = out.cpu().numpy()
        assert np.isfinite(out[:offs[-1]]).all() and np.isnan(out[offs[-1]:]).all()
        return [dict(samples=out[offs[i]:offs[i + 1]]) for i in range(len(rows))]

    with _det(hb, True):
        _invariance("resample", rows_, extra, run)


def test_reverb(hb):
    """Every row convolved with its own RIR (-1: copied by value), rir_index travelling with the utterance."""
    rows_, extra, banks = B.waves()
    plan = hb.ReverbPlan(banks["rirs"])

    def run(rows, name, ef, ec):
        c, samples, offsets = _packed(hb, rows, ef)
        total = int(c["offsets"][-1])
        out = torch.full((total + ef,), float("nan"), device=DEV)
        hb.reverb(plan, samples, offsets, _i32(hb, [w["rir"] for w in rows]), out, max_len=max(c["lens"]) + ef)
        out = out.cpu().numpy()
        assert np.isfinite(out[:total]).all() and np.isnan(out[total:]).all()
        for i, w in enumerate(rows):
            if w["rir"] < 0:
                assert np.array_equal(out[c["offsets"][i]:c["offsets"][i + 1]], w["x"])
        return [dict(samples=out[c["offsets"][i]:c["offsets"][i + 1]]) for i in range(len(rows))]

    with _det(hb, True):
        _invariance("reverb", rows_, extra, run)


def test_noise_mix(hb):
    """Every row plus its own clip from its own start at its own scale (-1: the row by value, gain 0); the mixed samples and
    the gain of every row."""
    rows_, extra, banks = B.waves()
    bank = hb.NoiseBank(banks["clips"])

    def run(rows, name, ef, ec):
        c, samples, offsets = _packed(hb, rows, ef)
        total = int(c["offsets"][-1])
        out = torch.full((total + ef,), float("nan"), device=DEV)
        gains = torch.full((len(rows),), float("nan"), device=DEV)
        hb.noise_mix(bank, samples, offsets, _i32(hb, [w["clip"] for w in rows]),
                     hb.to_device_i64([int(w["start"]) for w in rows], DEV),
                     hb.to_device_f32(np.array([w["scale"] for w in rows], dtype=np.float32), DEV), out=out,
                     max_len=max(c["lens"]) + ef, gains=gains)
        out, gains = out.cpu().numpy(), gains.cpu().numpy()
        assert np.isfinite(out[:total]).all() and np.isnan(out[total:]).all() and np.isfinite(gains).all()
        for i, w in enumerate(rows):
            if w["clip"] < 0:
                assert gains[i] == 0 and np.array_equal(out[c["offsets"][i]:c["offsets"][i + 1]], w["x"])
            else:
                assert gains[i] > 0
        return [dict(samples=out[c["offsets"][i]:c["offsets"][i + 1]], gain=gains[i:i + 1]) for i in range(len(rows))]

    with _det(hb, True):
        _invariance("noise_mix", rows_, extra, run)

"""The case tables of tests/test_batch_invariance_gpu.py, pinned without a GPU: the shapes sit where the kernels switch
(against the library's own limits), the moved order has no fixed point in row or graph index, and the float64 restatements
of the CTC loss, the alignment and the plain prefix beam search give every utterance the same result on the base batch and
on the moved one - so the builders of tests/batch_cases.py are shown to carry each utterance's data with it."""
import numpy as np
import torch
import torch.nn.functional as F

import batch_cases as B
import ctc_align_ref as A
import ctc_beam_ref as R
import hip_backend as hb


def test_beam_batches_sit_on_the_switches():
    lds, one_wave = hb.CTC_BEAM_LDS_ENTRIES, hb.CTC_BEAM_ONE_WAVE_KV
    a, b, c = B.BEAM["a"], B.BEAM["b"], B.BEAM["c"]
    assert (a["V"], a["K"], a["lens"]) == (34, 4, (0, 1, 7, 100))
    assert (b["V"], b["K"], b["lens"]) == (5, 16, (257, 256, 3, 0))
    assert (c["V"], c["K"], c["lens"]) == (260, 4, (7, 2))
    # (b): one row above and one row at the LDS limit; the batch's T K is above it, row 1's alone extent is not
    assert b["lens"][0] * b["K"] > lds and b["lens"][1] * b["K"] == lds
    assert max(b["lens"]) * b["K"] > lds and max(b["lens"][1], 1) * b["K"] <= lds
    assert b["extra"][0] > max(b["lens"])
    # (a) one wave with its history in LDS in every run, the moved one included; (c) four waves
    assert a["K"] * a["V"] <= one_wave and (max(a["lens"] + a["extra"][:1]) + B.EXTRA_FRAMES) * a["K"] <= lds
    assert b["K"] * b["V"] <= one_wave and c["K"] * c["V"] > one_wave
    for spec in (a, b, c):
        assert spec["extra"][0] > max(spec["lens"]) and len(spec["graph"]) == len(spec["lens"])
        assert -1 in spec["graph"] and {0, 1} <= set(spec["graph"] + spec["extra"][1:])
    assert set(B.MODES) == set(B.MODE_OUTPUTS) and len(B.MODES) == 6
    for mode, outs in B.MODE_OUTPUTS.items():
        assert outs[:3] == ("hyp", "hyp_len", "score") and ("ctx_score" in outs) == mode.startswith("context")
        assert ("n_words" in outs) == mode.startswith("word_lm") and ("lm_score" in outs) == (mode not in ("plain", "context"))


def test_ctc_label_counts_straddle_the_wave_and_the_workgroup():
    states = [2 * n + 1 for _, n in B.CTC_SHAPES]
    assert B.CTC_SHAPES == ((1, 0), (1, 1), (17, 0), (5, 4), (65, 31), (67, 32), (259, 128)) and B.CTC_V == 34
    assert 63 in states and 65 in states and max(s for s in states if s <= 64) == 63 and min(s for s in states if s > 64) == 65
    assert 257 in states and any(64 < s <= 256 for s in states)
    assert B.CTC_EXTRA[0] > max(t for t, _ in B.CTC_SHAPES)
    utts, extra = B.ctc_utts()
    assert [(u["z"].shape[0], len(u["y"])) for u in utts] == list(B.CTC_SHAPES) and extra["z"].shape[0] == B.CTC_EXTRA[0]
    y = utts[B.CTC_INFEASIBLE]["y"]
    assert len(y) + sum(p == q for p, q in zip(y, y[1:])) > utts[B.CTC_INFEASIBLE]["z"].shape[0]
    g = [u["g"] for u in utts]
    assert min(g) < 0 < max(g) and 0.0 in g
    al, _ = B.align_utts()
    assert len(al) == len(utts) and all(u is not utts[B.CTC_INFEASIBLE] for u in al)
    assert A.infeasible(al[-1]["z"].shape[0], len(al[-1]["y"])) or not A.align(al[-1]["z"].astype(np.float64), al[-1]["y"])["feasible"]


def test_the_other_case_tables_name_their_rows():
    utts, extra = B.rnnt_utts()
    assert [(u["z"].shape[0], len(u["y"])) for u in utts] == [(1, 0), (1, 1), (7, 0), (7, 3), (20, 9)]
    assert extra["z"].shape[0] > 20 and len(extra["y"]) > 9 and utts[0]["z"].shape[2] == 34 and B.RNNT_J % 4 == 0
    assert min(u["g"] for u in utts) < 0 < max(u["g"] for u in utts)
    mw, mx = B.mwer_utts()
    assert len(mw) == 3 and all(u["logits"].shape[1:] == (4, 34) for u in mw)
    npos = np.concatenate([u["npos"] for u in mw])
    assert 1 in npos and B.MWER_L in npos and 0 in npos and npos.max() == B.MWER_L and mx["npos"].max() > B.MWER_L
    assert len({u["logits"].shape[0] for u in mw}) > 1                     # an utterance whose own extent is shorter
    pairs, px = B.edit_pairs(hb.ED_MAX_COLS)
    assert len(pairs) == 8 and any(not p["hyp"] and not p["ref"] for p in pairs)
    assert any(not p["hyp"] and p["ref"] for p in pairs) and any(p["hyp"] and not p["ref"] for p in pairs)
    assert any(p["hyp"] and p["hyp"] == p["ref"] for p in pairs) and max(len(p["hyp"]) for p in pairs) == hb.ED_MAX_COLS
    assert len(px["hyp"]) == len(px["ref"]) == hb.ED_MAX_COLS > max(len(p["ref"]) for p in pairs)
    order = B.moved_ref_order(len(pairs))
    assert sorted(order) == list(range(9)) and all(r != i for i, r in enumerate(order))
    wv, wx, banks = B.waves()
    assert [w["x"].size for w in wv] == [1, 400, 1101] and wx["x"].size > 1101
    offs = B.waves_batch(wv)["offsets"]
    assert all(int(o) % 2 for o in offs[1:-1]) and B.waves_batch([wv[2]])["offsets"][0] == 0
    assert {w["rir"] for w in wv} == {-1, 0, 1} and {w["clip"] for w in wv} == {-1, 0, 1}
    assert len({w["factor"] for w in wv}) == 3 and len(banks["rirs"]) == 2 and len(banks["clips"]) == 2


def test_moved_order_has_no_fixed_point():
    for n in (2, 3, 4, 7, 8):
        order = B.moved_order(n)
        assert sorted(order) == [B.EXTRA] + list(range(n)) and all(b != r for r, b in enumerate(order))
    for name in sorted(B.BEAM):
        utts, extra, _ = B.beam_utts(name)
        runs = {a[0]: a for a in B.arrangements(utts, extra) if a[0] != "alone"}
        graphs, graph_of = B.graph_index(runs["moved"][1], "moved")
        assert graphs == [1, 0] and sum(g >= 0 for g in graph_of) >= 2
        assert all(g != r for r, g in enumerate(graph_of) if g >= 0), (name, graph_of)
        for r, u in enumerate(runs["moved"][1]):                           # the same graph behind another index
            assert graph_of[r] == -1 if u["graph"] < 0 else graphs[graph_of[r]] == u["graph"]
        assert B.graph_index(runs["base"][1], "base") == ([0, 1], [u["graph"] for u in utts])
        for u in utts:
            graphs, graph_of = B.graph_index([u], "alone")
            assert (graph_of == [-1]) if u["graph"] < 0 else (graph_of == [0] and graphs == [u["graph"]])
    names = [a[0] for a in B.arrangements(*B.ctc_utts())]
    assert names == ["base"] + ["alone"] * len(B.CTC_SHAPES) + ["moved", "padded"]


def _base_and_moved(utts, extra):
    runs = {a[0]: a for a in B.arrangements(utts, extra) if a[0] != "alone"}
    return runs["base"], runs["moved"]


def test_ctc_loss_restatement_follows_the_utterance():
    utts, extra = B.ctc_utts()
    got = {}
    for name, rows, owner, ef, ec in _base_and_moved(utts, extra):
        c = B.frames_batch(rows, ef, ec)
        z = torch.from_numpy(np.nan_to_num(c["buf"])).double().requires_grad_()
        nll = F.ctc_loss(F.log_softmax(z, -1).transpose(0, 1), torch.from_numpy(c["labels"]), torch.tensor(c["lens"]),
                         torch.tensor(c["label_lens"]), blank=0, reduction="none", zero_infinity=True)
        (nll * torch.from_numpy(c["g"]).double()).sum().backward()
        got[name] = {b: (float(nll[r].detach()), z.grad[r, :c["lens"][r]].numpy().copy()) for r, b in enumerate(owner) if b != B.EXTRA}
    assert sorted(got["base"]) == sorted(got["moved"]) == list(range(len(utts)))
    for b in got["base"]:
        assert got["base"][b][0] == got["moved"][b][0] and np.array_equal(got["base"][b][1], got["moved"][b][1]), b
    assert got["base"][B.CTC_INFEASIBLE][0] == 0.0 and all(got["base"][b][0] > 0 for b in got["base"] if b != B.CTC_INFEASIBLE)


def test_alignment_restatement_follows_the_utterance():
    utts, extra = B.align_utts()
    got = {}
    for name, rows, owner, ef, ec in _base_and_moved(utts, extra):
        c = B.frames_batch(rows, ef, ec)
        got[name] = {}
        for r, b in enumerate(owner):
            if b == B.EXTRA:
                continue
            zb = c["buf"][r, :c["lens"][r], :c["V"]].astype(np.float64)
            y = [int(v) for v in c["labels"][c["offsets"][r]:c["offsets"][r + 1]]]
            al = A.align(zb, y)
            tok, ids = A.best_path(zb) if zb.shape[0] else (np.zeros(0, int), ())
            got[name][b] = (al["feasible"], float(al["score"]) if al["feasible"] else None,
                            np.asarray(al["path"]).tolist() if al["feasible"] else None, np.asarray(tok).tolist(), list(ids))
    assert sorted(got["base"]) == sorted(got["moved"]) == list(range(len(utts)))
    assert got["base"] == got["moved"]
    assert [b for b, v in got["base"].items() if not v[0]] == [len(utts) - 1]


def test_beam_restatement_follows_the_utterance():
    for name in sorted(B.BEAM):
        utts, extra, _ = B.beam_utts(name)
        got = {}
        for arr, rows, owner, ef, ec in _base_and_moved(utts, extra):
            c = B.frames_batch(rows, ef, ec)
            got[arr] = {}
            for r, b in enumerate(owner):
                if b != B.EXTRA:
                    res = R.search(c["buf"][r, :c["lens"][r], :c["V"]].astype(np.float64), B.BEAM[name]["K"])
                    got[arr][b] = (res["hyps"], [float(s) for s in res["scores"]])
        assert sorted(got["base"]) == sorted(got["moved"]) == list(range(len(utts)))
        assert got["base"] == got["moved"], name
        assert all(len(v[0]) >= 1 for v in got["base"].values())

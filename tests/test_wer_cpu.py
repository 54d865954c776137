"""WER scoring, the parts that need no GPU: the plain-Python restatement of the word kernel (tests/wer_ref.py)
against str.split() of the reference-rendered strings of tests/golden/text.json, utils.calculate_wer, the host route of
utils.calculate_wer_ids, the `mwer_unit` key, and the new entry's declaration."""
import json
import os
import re

import pytest
import torch

import utils
import wer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(golden_dir):
    with open(os.path.join(golden_dir, "text.json")) as f:
        return json.load(f)


def _string_side(t, index=None):
    hyp = [h.split() for h in t["hyp"]]
    ref = [r.split() for r in t["ref"]]
    if index is not None:
        ref = [ref[i] for i in index]
    return [utils.edit_distance(h, r) for h, r in zip(hyp, ref)], [len(r) for r in ref]


def test_wer_ref_on_ids_is_split_on_the_rendered_strings(golden_dir):
    t = _text(golden_dir)
    vocab = t["vocab"]
    skip = utils.cer_token_table(vocab, t["non_lang_syms"]).tolist()
    dist, hyp_n, ref_n = wer_ref.word_edit_distance(t["preds"], t["refs"], vocab["<space>"], skip, vocab["<EOS>"])
    want_dist, want_n = _string_side(t)
    assert dist == want_dist and ref_n == want_n and hyp_n == [len(h.split()) for h in t["hyp"]]
    assert any("  " in h for h in t["hyp"]) and "" in t["hyp"], "the record holds a repeated space and an empty hypothesis"
    assert sum(dist) > 0
    # by hand: spaces at both ends and repeated, a dropped token inside a word and between spaces, <EOS> after a space
    A, B, S, N, E = vocab["a"], vocab["b"], vocab["<space>"], vocab["<NOISE>"], vocab["<EOS>"]
    assert wer_ref.words([S, S, A, N, B, S, S, N, S, B, S, E, A], S, skip, E) == [(A, B), (B,)]
    assert wer_ref.words([S, N, S], S, skip, E) == [] and wer_ref.words([], S, skip, E) == []
    assert wer_ref.words([A, B, E, B], S, skip) == [(A, B, B)], "references are never cut: their <EOS> is only dropped"


def test_calculate_wer_on_strings(golden_dir):
    t = _text(golden_dir)
    dist, ref_n = _string_side(t)
    assert utils.calculate_wer(t["hyp"], t["ref"]) == float(sum(dist)) / float(sum(ref_n))
    assert utils.calculate_wer(["the cat sat", " a  b "], ["the cat sat", "a c b"]) == 1.0 / 6.0
    assert utils.calculate_wer(["", "x y"], ["one two", "y"]) == 3.0 / 3.0


def test_calculate_wer_ids_host_route_is_the_string_path(golden_dir):
    t = _text(golden_dir)
    eos = t["vocab"]["<EOS>"]
    wer, dist, ref_n = utils.calculate_wer_ids(t["preds"], t["refs"], t["vocab"], t["non_lang_syms"], eos, torch.device("cpu"))
    want_dist, want_n = _string_side(t)
    assert (wer, dist, ref_n) == (utils.calculate_wer(t["hyp"], t["ref"]), want_dist, want_n)
    index = [1] * len(t["preds"])                                          # K hypotheses per reference
    wer_k, dist_k, ref_n_k = utils.calculate_wer_ids(t["preds"], t["refs"], t["vocab"], t["non_lang_syms"], eos, "cpu",
                                                      ref_index=index)
    want_dist, want_n = _string_side(t, index)
    assert (dist_k, ref_n_k) == (want_dist, want_n) and wer_k == float(sum(want_dist)) / float(sum(want_n))
    # a vocabulary without <space>: every sentence is one word, still the host's split()
    vocab = {k: v for k, v in t["vocab"].items() if k != "<space>"}
    ids = [[3, 4, 2], [5, 2]]
    assert utils.calculate_wer_ids(ids, [[3, 4], [3]], vocab, t["non_lang_syms"], eos, "cpu") == (0.5, [0, 1], [1, 1])


def test_mwer_unit_key():
    from solver import Solver
    vocab = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2, "a": 3, "<space>": 4}
    assert Solver.mwer_unit_config({}, vocab) is None and Solver.mwer_unit_config(dict(mwer_unit="token"), vocab) is None
    assert Solver.mwer_unit_config(dict(mwer_unit="word"), vocab) == 4
    assert Solver.mwer_unit_config(dict(mwer_unit="token"), {"a": 3}) is None
    for bad in ("char", "Word", None, 1):
        with pytest.raises(ValueError, match="mwer_unit"):
            Solver.mwer_unit_config(dict(mwer_unit=bad), vocab)
    with pytest.raises(ValueError, match="<space>"):
        Solver.mwer_unit_config(dict(mwer_unit="word"), {"<PAD>": 0, "a": 3})


def test_mwer_forward_refuses_a_unit_it_does_not_know():
    import model as M
    assert M.E2E.space_id is None
    net = M.E2E.__new__(M.E2E)
    net._beam_width = lambda beam: beam
    with pytest.raises(ValueError, match="unit"):
        M.E2E.mwer_forward(net, None, None, None, 2, unit="char")
    with pytest.raises(ValueError, match="space_id"):
        M.E2E.mwer_forward(net, None, None, None, 2, unit="word")


def test_header_declares_the_entry_and_the_binding_names_it():
    import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    decl = re.search(r"^int asr_word_edit_distance_i32\(([^;]*)\);", header, flags=re.M | re.S)
    assert decl, "asr_word_edit_distance_i32 is not declared"
    token = re.search(r"^int asr_edit_distance_i32\(([^;]*)\);", header, flags=re.M | re.S)
    norm = lambda m: re.sub(r"\s+", " ", m.group(1))
    assert norm(decl) == norm(token).replace("int V, ", "int V, int space, "), "the token entry's arguments plus `int space`"
    assert "asr_word_edit_distance_i32" in hb.EXPORTS and callable(hb.word_edit_distance)
    assert hb.ABI_VERSION == 8, "additive: no version change"

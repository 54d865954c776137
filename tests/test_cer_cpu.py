"""CER scoring from token ids, the parts that need no GPU: the skip table that says when edit distance on
ids equals edit distance on the rendered strings, the host route of calculate_cer_ids against the reference's own record
(tests/golden/text.json), and that the reference's Solver records (tests/golden/solver_run.json) can be scored from ids at
all - the GPU test pins the kernel against them."""
import json
import os

import numpy as np
import torch

import utils


def _text(golden_dir):
    with open(os.path.join(golden_dir, "text.json")) as f:
        return json.load(f)


def chars_to_ids(hyps, refs):
    """Strings -> id lists over an alphabet built from the strings themselves (one id per distinct character, from 3 up:
    0..2 stay <PAD>/<BOS>/<EOS>); (vocab, hyp ids, ref ids).  None when the strings do not map one to one - a character that
    to_sents could not have rendered from a single token."""
    chars = sorted(set("".join(hyps) + "".join(refs)))
    vocab = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2}
    for ch in chars:
        vocab["<space>" if ch == " " else ch] = len(vocab)
    if len(vocab) != 3 + len(chars):
        return None
    code = {ch: vocab["<space>" if ch == " " else ch] for ch in chars}
    return vocab, [[code[c] for c in h] for h in hyps], [[code[c] for c in r] for r in refs]


def test_token_table_of_the_text_vocabulary(golden_dir):
    t = _text(golden_dir)
    table = utils.cer_token_table(t["vocab"], t["non_lang_syms"])
    assert table.dtype == np.uint8 and table.shape == (len(t["vocab"]),)
    assert sorted(np.flatnonzero(table).tolist()) == sorted(t["vocab"][s] for s in t["non_lang_syms"])
    assert len(t["non_lang_syms"]) == 4 and int(table.sum()) == 4


def test_token_table_refuses_vocabularies_that_do_not_render_one_to_one(golden_dir):
    t = _text(golden_dir)
    nls = t["non_lang_syms"]
    with_unk = dict(t["vocab"], **{"<UNK>": len(t["vocab"])})                 # a kept multi-character token
    assert utils.cer_token_table(with_unk, nls) is None
    assert utils.cer_token_table(with_unk, nls + ["<UNK>"]) is not None       # ... dropped before scoring: fine
    assert utils.cer_token_table(dict(t["vocab"], **{" ": len(t["vocab"])}), nls) is None    # <space> and " ": one character
    assert utils.cer_token_table(t["vocab"], [s for s in nls if s != "<EOS>"]) is None       # a kept <EOS> renders 5 characters


def test_calculate_cer_ids_host_route_reproduces_the_reference_record(golden_dir):
    t = _text(golden_dir)
    eos = t["vocab"]["<EOS>"]
    cer, dist, ref_n = utils.calculate_cer_ids(t["preds"], t["refs"], t["vocab"], t["non_lang_syms"], eos, torch.device("cpu"))
    assert abs(cer - t["cer"]) <= 1e-12
    assert cer == utils.calculate_cer(t["hyp"], t["ref"])
    assert dist == [utils.edit_distance(h, r) for h, r in zip(t["hyp"], t["ref"])] and ref_n == [len(r) for r in t["ref"]]
    # K hypotheses per reference: every prediction against reference 1
    cer_k, dist_k, ref_n_k = utils.calculate_cer_ids(t["preds"], t["refs"], t["vocab"], t["non_lang_syms"], eos, "cpu",
                                                      ref_index=[1] * len(t["preds"]))
    assert dist_k == [utils.edit_distance(h, t["ref"][1]) for h in t["hyp"]] and ref_n_k == [len(t["ref"][1])] * len(t["preds"])
    assert cer_k == float(sum(dist_k)) / float(sum(ref_n_k))


def test_solver_run_records_can_be_scored_from_ids(golden_dir):
    """Every sup[*] record of the reference's Solver run maps to ids one to one (at most one record in ten may fail to), and
    its recorded CER is calculate_cer of its strings - what the GPU test then asks of the kernel."""
    with open(os.path.join(golden_dir, "solver_run.json")) as f:
        records = json.load(f)["sup"]
    skipped = 0
    for rec in records:
        mapped = chars_to_ids(rec["hyps"], rec["refs"])
        if mapped is None:
            skipped += 1
            continue
        vocab, hyp_ids, ref_ids = mapped
        assert utils.cer_token_table(vocab, ["<PAD>", "<BOS>", "<EOS>"]) is not None
        assert utils.to_sents(hyp_ids, vocab, ["<PAD>", "<BOS>", "<EOS>"]) == rec["hyps"]
        assert abs(utils.calculate_cer(rec["hyps"], rec["refs"]) - rec["cer"]) <= 1e-12
    assert len(records) >= 10 and skipped * 10 <= len(records), (skipped, len(records))
    assert max(rec["cer"] for rec in records) > 1.0                            # long hypotheses are among them

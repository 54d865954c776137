"""The word-level edit distance of csrc/edit_distance.hip (asr_word_edit_distance_i32) restated in plain Python:
cut the hypothesis before its first <EOS>, drop the tokens of the skip table from both sides, split at `space` into tuples of
ids, utils.edit_distance on the two lists of tuples.  No GPU code; the tests' yardstick."""
import utils


def words(row, space, skip=(), eos=-1):
    """The words of one row of ids, as tuples: [A, B, space, space, C] -> [(A, B), (C,)]."""
    row = [int(t) for t in row]
    if eos >= 0 and eos in row:
        row = row[:row.index(eos)]
    out, cur = [], []
    for t in row:
        if 0 <= t < len(skip) and skip[t]:
            continue
        if t == space:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(t)
    if cur:
        out.append(tuple(cur))
    return out


def word_edit_distance(hyps, refs, space, skip=(), eos=-1, ref_index=None):
    """-> (dist, hyp_n, ref_n), three lists over the pairs: hypothesis p (cut at `eos`) against reference p, or
    ref_index[p] (never cut)."""
    index = range(len(hyps)) if ref_index is None else ref_index
    hw = [words(h, space, skip, eos) for h in hyps]
    rw = [words(refs[int(r)], space, skip) for r in index]
    return [utils.edit_distance(h, r) for h, r in zip(hw, rw)], [len(h) for h in hw], [len(r) for r in rw]

"""Host-side helpers on the training path, same names/semantics as the reference's utils.py
(cc 150-152, to_gpu 154-158, pad_list 173-179, _seq_mask 181-190, adjust_learning_rate 134-139,
remove_pad_eos 192-201, to_sents/ind2character/char_list_to_str 160-163,212-235, calculate_cer
222-228, Logger 237-245, infinite_iter 247-254).  tensorboardX and editdistance are optional:
absent here, so logging degrades to a no-op and the edit distance is computed locally - on the host (edit_distance), or for
whole sets of hypotheses on the GPU (calculate_cer_ids, calculate_wer_ids; not reference functions: cer_token_table,
calculate_cer_ids, calculate_wer, calculate_wer_ids).
"""
import numpy as np
import torch

try:  # optional dependency (not installed in the ROCm image)
    from tensorboardX import SummaryWriter as _SummaryWriter
except Exception:  # pragma: no cover
    _SummaryWriter = None


def cc(net):
    """Move a module/tensor to the GPU when there is one ('cuda' is HIP on ROCm)."""
    return net.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))


def to_gpu(data):
    xs, ilens, ys = data
    return cc(xs), ilens, [cc(y) for y in ys]


def pad_list(xs, pad_value=0):
    """Ragged list of tensors -> [B, Lmax, ...] filled with pad_value."""
    longest = max(int(x.size(0)) for x in xs)
    out = xs[0].new_full((len(xs), longest) + tuple(xs[0].shape[1:]), pad_value)
    for i, x in enumerate(xs):
        out[i, : x.size(0)] = x
    return out


def _seq_mask(seq_len, max_len, is_list=True):
    """Float mask [B, max_len]: 1 where position < length."""
    lens = torch.as_tensor(np.asarray(seq_len)) if is_list else seq_len
    grid = torch.arange(0, max_len, device=lens.device).unsqueeze(0)
    return (grid < lens.unsqueeze(1)).float()


def adjust_learning_rate(optimizer, lr):
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def remove_pad_eos(sequences, eos=2):
    """Keep each sequence up to (excluding) its first <EOS>."""
    out = []
    for seq in sequences:
        seq = list(seq)
        out.append(seq[: seq.index(eos)] if eos in seq else seq)
    return out


def ind2character(sequences, non_lang_syms, vocab):
    inv = {v: k for k, v in vocab.items()}
    skip = set(vocab[s] for s in non_lang_syms)
    return [[inv[int(i)] for i in seq if int(i) not in skip] for seq in sequences]


def char_list_to_str(char_lists):
    return ["".join(" " if ch == "<space>" else ch for ch in chars) for chars in char_lists]


def to_sents(ind_seq, vocab, non_lang_syms):
    return char_list_to_str(ind2character(ind_seq, non_lang_syms, vocab))


def edit_distance(a, b):
    """Levenshtein distance (stands in for editdistance.eval)."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def calculate_cer(hyps, refs):
    total_dis = sum(edit_distance(h, r) for h, r in zip(hyps, refs))
    total_len = sum(len(r) for r in refs)
    return float(total_dis) / float(total_len)


def cer_token_table(vocab, non_lang_syms):
    """uint8 [V] skip table (1: the id is a non-language symbol, dropped before scoring) when edit distance on token ids
    equals edit distance on the strings to_sents renders - every kept token renders to exactly one character (<space> to
    " ") and distinct kept ids render to distinct characters; None otherwise ("score on the host": e.g. a kept <UNK>)."""
    inv = {int(v): k for k, v in vocab.items()}
    skip = set(int(vocab[s]) for s in non_lang_syms)
    if not inv or min(inv) < 0:
        return None
    table = np.zeros(max(inv) + 1, dtype=np.uint8)
    seen = set()
    for i, sym in inv.items():
        if i in skip:
            table[i] = 1
            continue
        ch = " " if sym == "<space>" else sym
        if len(ch) != 1 or ch in seen:
            return None
        seen.add(ch)
    return table


_SKIP_TABLES = {}          # (device, table bytes) -> the table on that device


def _device_score(hyp_ids, ref_ids, table, eos, device, ref_index, space=None):
    """One upload (both id matrices, their lengths and the reference index in one int32 buffer), one launch of
    asr_edit_distance_i32 - with `space`, of asr_word_edit_distance_i32 -, one read-back -> (sum dist, sum ref_n, dist,
    ref_n); None when the kernel declines the shape."""
    import hip_backend as hb
    n, nr = len(hyp_ids), len(ref_ids)
    if n == 0 or nr == 0:
        return None
    lh = max(1, max(len(h) for h in hyp_ids))
    lr = max(1, max(len(r) for r in ref_ids))
    if max(lh, lr) > hb.ED_MAX_COLS:
        return None
    sizes = (n * lh, n, nr * lr, nr, n if ref_index is not None else 0)
    host = np.zeros(sum(sizes), dtype=np.int32)
    hyp, hyp_len, ref, ref_len, index = np.split(host, np.cumsum(sizes)[:-1])
    hyp, ref = hyp.reshape(n, lh), ref.reshape(nr, lr)
    for rows, lens, seqs in ((hyp, hyp_len, hyp_ids), (ref, ref_len, ref_ids)):
        for i, seq in enumerate(seqs):
            rows[i, :len(seq)] = seq
            lens[i] = len(seq)
    if ref_index is not None:
        index[:] = ref_index
    dev = torch.from_numpy(host).to(device)
    d_hyp, d_hyp_len, d_ref, d_ref_len, d_index = torch.split(dev, sizes)
    key = (str(device), table.tobytes())
    if key not in _SKIP_TABLES:
        _SKIP_TABLES[key] = torch.from_numpy(table).to(device)
    res = torch.zeros(4 + 3 * n, dtype=torch.int32, device=device)       # the two 64-bit totals, then dist | hyp_n | ref_n
    try:
        kw = dict(hyp_len=d_hyp_len, ref_index=d_index if ref_index is not None else None, eos=eos, skip=_SKIP_TABLES[key],
                  totals=res[:4].view(torch.int64), out=res[4:].view(3, n))
        if space is None:
            hb.edit_distance(d_hyp.view(n, lh), d_ref.view(nr, lr), d_ref_len, **kw)
        else:
            hb.word_edit_distance(d_hyp.view(n, lh), d_ref.view(nr, lr), d_ref_len, space, **kw)
    except hb.UnsupportedShape:
        return None
    got = res.cpu().numpy()
    total_dis, total_len = (int(v) for v in got[:4].view(np.int64))
    rows = got[4:].reshape(3, n)
    return total_dis, total_len, rows[0].tolist(), rows[2].tolist()


def calculate_cer_ids(hyp_ids, ref_ids, vocab, non_lang_syms, eos, device, ref_index=None):
    """calculate_cer from token ids, scored on the GPU (csrc/edit_distance.hip, one launch per call): hyp_ids are cut before
    their first `eos` and both sides lose the non-language symbols, as remove_pad_eos + to_sents do; pair p scores against
    ref_ids[p], or ref_ids[ref_index[p]] (K hypotheses per reference).  -> (cer, dist, ref_n): cer = float(sum dist) /
    float(sum ref_n) from the integer totals - the same double calculate_cer forms on the strings - and the per-pair
    distances and reference lengths as host lists.  On a CPU device, for a vocabulary whose ids and characters do not
    correspond one to one (cer_token_table) or beyond the kernel's limits the same three values come from the host loop."""
    device = torch.device(device)
    table = cer_token_table(vocab, non_lang_syms) if device.type == "cuda" else None
    got = _device_score(hyp_ids, ref_ids, table, eos, device, ref_index) if table is not None else None
    if got is None:
        hyps = to_sents(remove_pad_eos(hyp_ids, eos=eos), vocab, non_lang_syms)
        refs = to_sents(ref_ids, vocab, non_lang_syms)
        if ref_index is not None:
            refs = [refs[int(i)] for i in ref_index]
        dist = [edit_distance(h, r) for h, r in zip(hyps, refs)]
        ref_n = [len(r) for r in refs]
        got = sum(dist), sum(ref_n), dist, ref_n
    total_dis, total_len, dist, ref_n = got
    return float(total_dis) / float(total_len), dist, ref_n


def calculate_wer(hyps, refs):
    """Word error rate of strings: calculate_cer over their words (str.split())."""
    return calculate_cer([h.split() for h in hyps], [r.split() for r in refs])


def calculate_wer_ids(hyp_ids, ref_ids, vocab, non_lang_syms, eos, device, ref_index=None):
    """calculate_wer from token ids, scored on the GPU (asr_word_edit_distance_i32, one launch per call): the
    arguments and the pairing are calculate_cer_ids'.  -> (wer, dist, ref_n): wer = float(sum dist) / float(sum ref_n), the
    per-pair word distances and the references' word counts as host lists.  The device scores when ids and characters
    correspond one to one (cer_token_table) and <space> is a kept id; on a CPU device, without such a table or <space>, or
    beyond the kernel's limits the same three values come from the host loop over the words of the rendered strings."""
    device = torch.device(device)
    table = cer_token_table(vocab, non_lang_syms) if device.type == "cuda" else None
    space = vocab.get("<space>")
    got = None
    # (str.split() also cuts at any other white-space character: a vocabulary that keeps one is scored on the host)
    if (table is not None and space is not None and table[int(space)] == 0
            and not any(s.isspace() for s, i in vocab.items() if table[int(i)] == 0)):
        got = _device_score(hyp_ids, ref_ids, table, eos, device, ref_index, space=int(space))
    if got is None:
        hyps = [h.split() for h in to_sents(remove_pad_eos(hyp_ids, eos=eos), vocab, non_lang_syms)]
        refs = [r.split() for r in to_sents(ref_ids, vocab, non_lang_syms)]
        if ref_index is not None:
            refs = [refs[int(i)] for i in ref_index]
        dist = [edit_distance(h, r) for h, r in zip(hyps, refs)]
        ref_n = [len(r) for r in refs]
        got = sum(dist), sum(ref_n), dist, ref_n
    total_dis, total_len, dist, ref_n = got
    return float(total_dis) / float(total_len), dist, ref_n


class Logger(object):
    """tensorboardX scalar/text logger; silently inert when tensorboardX is not installed."""

    def __init__(self, logdir="./log"):
        self.writer = _SummaryWriter(logdir) if _SummaryWriter is not None else None

    def scalar_summary(self, tag, value, step):
        if self.writer is not None:
            self.writer.add_scalar(tag, value, step)

    def text_summary(self, tag, value, step):
        if self.writer is not None:
            self.writer.add_text(tag, value, step)


def infinite_iter(iterable):
    while True:
        for item in iterable:
            yield item

"""A word-level backoff n-gram LM behind a lexicon, for character models: what the CTC prefix beam search
(csrc/ctc_beam.hip) and the scoring kernel (csrc/word_lm.hip) walk.  numpy only; nothing of the GPU path is imported here
(WordLM.to imports torch where it is called).

  Lexicon(words, vocab, space, bos, eos)            a word list spelled in token ids; compiles to a trie
  WordLM.from_arpa(path_or_text, vocab, space, lexicon=None)   a standard ARPA file over words
  WordLM.estimate(token_rows, space, order)         Witten-Bell over the words of token rows (NgramLM.estimate over word ids)
  lm.score(ids, eos_term=True)                      float64, by explicit backoff (NgramLM.score over the row's word ids)
  lm.compile() -> WordTable                         the sparse device form; lm.to(device) uploads it once

On the host the model IS an ngram.NgramLM over word ids: 0 is kept free (as the blank is among tokens), 1 = <s>, 2 = </s>,
3 = <unk>, 4 .. the words.  The words of a token row are tests/wer_ref.py's: split at <space>, a run of spaces is one
boundary, leading and trailing spaces make no word.  A word that is not in the lexicon is <unk>; if <unk> has no unigram it
scores oov_logp and the word state goes to the empty context (NgramLM's rule for a token without a unigram)."""
import math
import os

import numpy as np

from ngram import NgramLM

W_BOS, W_EOS, W_UNK, W_FIRST = 1, 2, 3, 4
UNK_NAMES = ("<unk>", "<UNK>")


def split_words(row, space):
    """The words of one row of token ids, as tuples: [A, B, space, space, C] -> [(A, B), (C,)]."""
    out, cur = [], []
    for t in row:
        t = int(t)
        if t == space:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(t)
    if cur:
        out.append(tuple(cur))
    return out


class Lexicon(object):
    """A list of words, each spelled as a tuple of token ids.  words: strings (spelled by characters through vocab, {symbol:
    token id}) or tuples of ids.  No id may be the blank (0), <space>, <BOS> or <EOS>; a word with a character outside the
    vocabulary is a ValueError that names it; a word listed twice counts once.  bos / eos None: the token vocabulary has no
    such id (a bare CTC head over letters)."""

    def __init__(self, words, vocab=None, space=None, bos=None, eos=None, V=None):
        self.space = int(space)
        self.bos, self.eos = (None if bos is None else int(bos)), (None if eos is None else int(eos))
        self.V = int(V) if V is not None else max(int(i) for i in vocab.values()) + 1
        if not 0 < self.space < self.V:
            raise ValueError("<space> = %d is not a token of 1 .. %d" % (self.space, self.V - 1))
        self.spellings, self.names, self.index = [], [], {}
        banned = {0, self.space, self.bos, self.eos}
        for word in words:
            if isinstance(word, str):
                if any(ch not in vocab for ch in word):
                    raise ValueError("lexicon: the word %r has a character outside the vocabulary" % (word,))
                ids = tuple(int(vocab[ch]) for ch in word)
            else:
                ids = tuple(int(i) for i in word)
            if not ids or any(i in banned or not 0 < i < self.V for i in ids):
                raise ValueError("lexicon: the word %r is empty or holds the blank, <space>, <BOS>, <EOS> or an id outside "
                                 "1 .. %d" % (word, self.V - 1))
            if ids not in self.index:
                self.index[ids] = len(self.spellings)
                self.spellings.append(ids)
                self.names.append(word if isinstance(word, str) else " ".join(str(i) for i in ids))

    def __len__(self):
        return len(self.spellings)

    def compile(self, word_ids=None):
        """-> (trie_next int32 [N, V]: the child node or -1, node 0 the root; trie_word int32 [N]: the word that ends at the
        node - its position in the list, or word_ids[position] - or -1)."""
        kids, word = [{}], [-1]
        for i, ids in enumerate(self.spellings):
            node = 0
            for c in ids:
                if c not in kids[node]:
                    kids[node][c] = len(kids)
                    kids.append({})
                    word.append(-1)
                node = kids[node][c]
            word[node] = i if word_ids is None else int(word_ids[i])
        if len(kids) * self.V >= 2 ** 31:
            raise ValueError("the trie has %d nodes x %d tokens: N V must stay below 2**31" % (len(kids), self.V))
        nxt = np.full((len(kids), self.V), -1, dtype=np.int32)
        for node, d in enumerate(kids):
            for c, child in d.items():
                nxt[node, c] = child
        return nxt, np.array(word, dtype=np.int32)


class WordTable(object):
    """The compiled device form (include/asr_hip.h, asr_word_lm_t).  On the host the arrays are numpy, after .to(device)
    device tensors.  FIELDS in the order of the struct's pointers."""
    FIELDS = ("trie_next", "trie_word", "arc_off", "arc_word", "arc_logp", "arc_next", "bo_logp", "bo_state", "uni_logp", "uni_next")

    def __init__(self, arrays, V, space, start, empty, eos, unk, order):
        for k in self.FIELDS:
            setattr(self, k, arrays[k])
        self.V, self.space, self.start, self.empty, self.eos, self.unk, self.order = int(V), int(space), int(start), int(empty), \
            int(eos), int(unk), int(order)
        self.N, self.S, self.W = int(self.trie_word.shape[0]), int(self.bo_state.shape[0]), int(self.uni_next.shape[0])
        self.A = int(arrays["n_arcs"])
        self.exact = arrays.get("exact")                         # (host only) the float64 values the float32 ones were rounded from

    def arrays(self):
        d = {k: getattr(self, k) for k in self.FIELDS}
        d["n_arcs"] = self.A
        return d

    def to(self, device):
        import torch
        d = {}
        for k in self.FIELDS:
            a = getattr(self, k)
            d[k] = a.to(device) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(device)
        d["n_arcs"] = self.A
        return WordTable(d, self.V, self.space, self.start, self.empty, self.eos, self.unk, self.order)

    def lookup(self, s, w, dt=np.float64, exact=False):
        """The kernels' lookup on the host arrays, in dtype dt, every addition rounded on its own -> (lp, next state).
        exact: over the float64 values the table was rounded from."""
        arc_logp, bo_logp, uni_logp = self.exact if exact else (self.arc_logp, self.bo_logp, self.uni_logp)
        if self.uni_next[w] < 0:
            return dt(uni_logp[w]), self.empty
        acc = dt(0)
        while s != self.empty:
            lo, hi = int(self.arc_off[s]), int(self.arc_off[s + 1])
            at = lo + int(np.searchsorted(self.arc_word[lo:hi], w))
            if at < hi and self.arc_word[at] == w:
                return dt(acc + dt(arc_logp[at])), int(self.arc_next[at])
            acc = dt(acc + dt(bo_logp[s]))
            s = int(self.bo_state[s])
        return dt(acc + dt(uni_logp[w])), int(self.uni_next[w])


class WordLM(object):
    """lm: an ngram.NgramLM over word ids (bos = 1, eos = 2; V = W); lexicon: the Lexicon whose word i has the id
    word_ids[i] (default 4 + i).  bos / eos / space / V here are TOKEN ids and the token vocabulary's size: what a decoder
    checks against its own."""

    def __init__(self, lm, lexicon, word_ids=None):
        self.lm, self.lexicon = lm, lexicon
        self.word_ids = [W_FIRST + i for i in range(len(lexicon))] if word_ids is None else [int(i) for i in word_ids]
        if (lm.bos, lm.eos) != (W_BOS, W_EOS):
            raise ValueError("the word LM keeps <s> = %d and </s> = %d, got %d and %d" % (W_BOS, W_EOS, lm.bos, lm.eos))
        if len(self.word_ids) != len(lexicon) or any(not W_FIRST <= i < lm.V for i in self.word_ids) or \
                len(set(self.word_ids)) != len(self.word_ids):
            raise ValueError("the lexicon's word ids must be distinct ids in %d .. W - 1 = %d" % (W_FIRST, lm.V - 1))
        self.V, self.space, self.bos, self.eos = lexicon.V, lexicon.space, lexicon.bos, lexicon.eos
        self.W, self.order, self.oov_logp = lm.V, lm.order, lm.oov_logp
        self._id_of = {ids: self.word_ids[i] for ids, i in lexicon.index.items()}
        self._table = None
        self._device = {}

    # ------------------------------------------------------------------------------------------------------------ ARPA
    @classmethod
    def from_arpa(cls, path_or_text, vocab, space, lexicon=None, bos=None, eos=None, oov_logp=-30.0, V=None):
        """path_or_text: an ARPA file over words (a file name, or the text).  vocab: {symbol: token id}, the characters the
        words are spelled in; space: the token id of <space>; bos / eos: the token ids of <BOS> / <EOS> (default: vocab's,
        if it has them).  lexicon: a Lexicon, or a list of words - the words the search may spell; default: the ARPA
        unigrams.  An ARPA word outside a given lexicon keeps its n-grams (it can only be reached as context, never
        spelled); a lexicon word outside the ARPA file has no unigram and scores oov_logp."""
        text = path_or_text
        if "\n" not in text:
            with open(os.fspath(path_or_text), "r", encoding="utf-8") as f:
                text = f.read()
        bos = vocab.get("<BOS>") if bos is None else int(bos)
        eos = vocab.get("<EOS>") if eos is None else int(eos)
        V = max(int(i) for i in vocab.values()) + 1 if V is None else int(V)
        listed, section = [], 0
        for raw in text.splitlines():
            line = raw.strip()
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:-7])
            elif line == "\\end\\":
                break
            elif section == 1 and line:
                f = line.split()
                if len(f) >= 2 and f[1] not in ("<s>", "</s>") + UNK_NAMES:
                    listed.append(f[1])
        if lexicon is None:
            lexicon = Lexicon(listed, vocab, space, bos, eos, V=V)
        elif not isinstance(lexicon, Lexicon):
            lexicon = Lexicon(list(lexicon), vocab, space, bos, eos, V=V)
        words = {name: W_UNK for name in UNK_NAMES}
        for i, name in enumerate(lexicon.names):
            words[name] = W_FIRST + i
        n = W_FIRST + len(lexicon)
        for name in listed:
            if name not in words:
                words[name] = n
                n += 1
        lm = NgramLM.from_arpa(text, words, W_BOS, W_EOS, oov_logp=oov_logp, V=n)
        return cls(lm, lexicon)

    # ------------------------------------------------------------------------------------------------------- estimation
    @classmethod
    def estimate(cls, token_rows, space, order, V=None, bos=None, eos=None, oov_logp=-30.0):
        """Witten-Bell (NgramLM.estimate) over the words of token rows; the lexicon is the words seen, in sorted order.
        V: the token vocabulary's size (default: the greatest id seen + 1, at least space + 1).  <unk> is an event of the
        estimate like every word id, so it has a unigram."""
        rows = [split_words(r, space) for r in token_rows]
        seen = sorted({w for r in rows for w in r})
        if V is None:
            V = max([int(space), int(bos or 0), int(eos or 0)] + [c for w in seen for c in w]) + 1
        lexicon = Lexicon(seen, None, space, bos, eos, V=V)
        ids = [[W_FIRST + lexicon.index[w] for w in r] for r in rows]
        return cls(NgramLM.estimate(ids, order, W_FIRST + len(lexicon), W_BOS, W_EOS, oov_logp=oov_logp), lexicon)

    # ------------------------------------------------------------------------------------------------- host evaluation
    def word_ids_of(self, ids):
        """The word ids of a token row; a word outside the lexicon is <unk>."""
        return [self._id_of.get(w, W_UNK) for w in split_words(ids, self.space)]

    def score(self, ids, eos_term=True):
        """float64, by explicit backoff over the row's word ids (no automaton, no table)."""
        return self.lm.score(self.word_ids_of(ids), eos_term)

    def n_words(self, ids):
        return len(split_words(ids, self.space))

    # ----------------------------------------------------------------------------------------------------- device form
    def compile(self):
        """-> WordTable, computed once: the trie, the arcs of every state in CSR form (words ascending), the backoff of
        every state, the direct-indexed empty context.  Values are the float64 ones rounded to float32 once.  Validated
        here - the kernels trust the tables: every node, state and word index in range, every value finite, every backoff
        chain ends at the empty context, N V and A below 2**31."""
        if self._table is not None:
            return self._table
        lm = self.lm
        states = lm.states()
        index = {s: i for i, s in enumerate(states)}
        S, W, lim = len(states), lm.V, lm.order - 1
        empty = index[()]

        def state_of(g):                                         # the longest suffix of g (at most order - 1 long) that is a state
            g = g[max(0, len(g) - lim):] if lim > 0 else ()
            while g not in index:
                g = g[1:]
            return index[g]
        has_uni = np.zeros(W, dtype=bool)
        uni_logp = np.full(W, lm.oov_logp, dtype=np.float64)
        uni_next = np.full(W, -1, dtype=np.int64)
        for g, p in lm.prob.items():
            if len(g) == 1:
                has_uni[g[0]] = True
                uni_logp[g[0]] = p
                uni_next[g[0]] = state_of(g)
        listed = {}
        for g, p in lm.prob.items():
            if len(g) >= 2 and has_uni[g[-1]]:
                listed.setdefault(g[:-1], []).append((g[-1], p, state_of(g)))
        arcs, ctx = [dict() for _ in range(S)], []
        bo_logp, bo_state = np.zeros(S, dtype=np.float64), np.full(S, empty, dtype=np.int64)
        for i, s in enumerate(states):
            h = s[max(0, len(s) - lim):] if lim > 0 else ()
            ctx.append(h)
            if len(h) >= 1:
                arcs[i] = {w: (p, nx) for w, p, nx in listed.get(h, ())}
                bo_logp[i] = lm.backoff.get(h, 0.0)
                base = h[1:]
                while base not in index:
                    base = base[1:]
                bo_state[i] = index[base]
        # a model given as dictionaries may hold a state h . w whose n-gram is not listed (an ARPA file lists every prefix of
        # what it lists): the backoff chain would pass it by, so the state gets an arc with the resolved value
        children = {}
        for s in index:
            if len(s) >= 1:
                children.setdefault(s[:-1], set()).add(s[-1])

        def path_next(i, w):
            while i != empty:
                if w in arcs[i]:
                    return arcs[i][w][1]
                i = int(bo_state[i])
            return int(uni_next[w])
        for i in sorted(range(S), key=lambda i: (len(ctx[i]), i)):
            h = ctx[i]
            for j in range(len(h)):
                if len(h) - j + 1 > lim:
                    continue
                for w in sorted(children.get(h[j:], ())):
                    if has_uni[w] and w not in arcs[i] and path_next(i, w) != state_of(h + (w,)):
                        arcs[i][w] = (lm.token_logp(h, w), state_of(h + (w,)))
        arc_off = np.zeros(S + 1, dtype=np.int64)
        arc_word, arc_logp, arc_next = [], [], []
        for i in range(S):
            for w in sorted(arcs[i]):
                arc_word.append(w), arc_logp.append(arcs[i][w][0]), arc_next.append(arcs[i][w][1])
            arc_off[i + 1] = len(arc_word)
        A = len(arc_word)
        trie_next, trie_word = self.lexicon.compile(self.word_ids)
        N = trie_word.shape[0]
        if A >= 2 ** 31 or N * self.V >= 2 ** 31:
            raise ValueError("the word LM has %d arcs and %d x %d trie entries: both must stay below 2**31" % (A, N, self.V))
        arrays = dict(trie_next=trie_next, trie_word=trie_word, arc_off=arc_off.astype(np.int32),
                      arc_word=np.array(arc_word + [0] * (A == 0), dtype=np.int32),
                      arc_logp=np.array(arc_logp + [0.0] * (A == 0), dtype=np.float64).astype(np.float32),
                      arc_next=np.array(arc_next + [0] * (A == 0), dtype=np.int32), bo_logp=bo_logp.astype(np.float32),
                      bo_state=bo_state.astype(np.int32), uni_logp=uni_logp.astype(np.float32), uni_next=uni_next.astype(np.int32),
                      n_arcs=A, exact=(np.array(arc_logp + [0.0] * (A == 0), dtype=np.float64), bo_logp, uni_logp))
        table = WordTable(arrays, self.V, self.space, index[(lm.bos,)], empty, W_EOS, W_UNK, lm.order)
        self.check_table(table)
        self._table = table
        return table

    @staticmethod
    def check_table(t):
        """ValueError unless the kernels can trust t (host arrays)."""
        A, S, W, N, V = t.A, t.S, t.W, t.N, t.V
        ok = t.trie_next.shape == (N, V) and t.trie_next.min() >= -1 and t.trie_next.max() < N
        ok = ok and t.trie_word.min() >= -1 and t.trie_word.max() < W
        ok = ok and t.arc_off.shape == (S + 1,) and t.arc_off[0] == 0 and t.arc_off[S] == A and (np.diff(t.arc_off) >= 0).all()
        if A:
            ok = ok and t.arc_word[:A].min() >= 0 and t.arc_word[:A].max() < W and t.arc_next[:A].min() >= 0 and \
                t.arc_next[:A].max() < S and (t.uni_next[t.arc_word[:A]] >= 0).all()
            rising = np.diff(t.arc_word[:A].astype(np.int64)) > 0
            starts = np.zeros(A, dtype=bool)
            starts[t.arc_off[1:S][t.arc_off[1:S] < A]] = True
            ok = ok and bool((rising | starts[1:]).all())
        ok = ok and t.bo_state.min() >= 0 and t.bo_state.max() < S and t.uni_next.min() >= -1 and t.uni_next.max() < S
        ok = ok and 0 <= t.start < S and 0 <= t.empty < S and 0 <= t.eos < W and 0 <= t.unk < W and 0 < t.space < V
        if not ok:
            raise ValueError("the word LM's tables hold an index out of range or arcs out of order")
        for a in (t.arc_logp, t.bo_logp, t.uni_logp):
            if not np.isfinite(a).all():
                raise ValueError("the word LM's tables hold a log-probability that is not finite")
        at = np.arange(S)                                        # every backoff chain reaches the empty context
        for _ in range(max(t.order, 1) + 1):
            at = np.where(at == t.empty, at, t.bo_state[at])
        if (at != t.empty).any():
            raise ValueError("a backoff chain of the word LM does not end at the empty context")

    def to(self, device):
        """The compiled tables on `device`, uploaded once per device."""
        key = str(device)
        if key not in self._device:
            self._device[key] = self.compile().to(device)
        return self._device[key]

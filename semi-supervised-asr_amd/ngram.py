"""A backoff n-gram language model over label ids: the one LM cheap enough to sit inside the CTC prefix beam
search - with the backoffs resolved on the host it is two table reads per (prefix, token).  numpy only; nothing of the GPU
path is imported here (NgramLM.to imports torch where it is called).

  NgramLM.from_arpa(path_or_text, vocab, bos, eos)    a standard ARPA file; log10 -> natural log in float64
  NgramLM.estimate(id_sequences, order, V, bos, eos)  interpolated Witten-Bell from transcripts, written in backoff form
  lm.to_arpa(symbols=None)                            the model as ARPA text
  lm.score(ids, eos_term=True)                        float64, by explicit backoff - no automaton
  lm.compile() -> NgramTable                          the deterministic automaton the kernels walk (logp fp32 [S, V], next
                                                      int32 [S, V], start); lm.to(device) uploads it once

Conventions: a sentence is scored from the context (<s>) - ONE <s>, not order - 1 of them; id 0 is the CTC blank (<PAD>)
and carries nothing; a token without a unigram (<s> among them: its ARPA unigram only carries the backoff of the start
context) scores `oov_logp` whatever the context."""
import math
import os

import numpy as np

LN10 = math.log(10.0)
ARPA_NO_PROB = -99.0          # log10: the conventional "probability" of <s>, which is a context and never predicted


class NgramTable(object):
    """The compiled automaton: logp float32 [S, V] (natural log of p(c | state) after backoff; column 0 holds 0), nxt int32
    [S, V] (the state after c), start (the state of <s>), and logp64, the float64 values logp was rounded from (once).
    On the host these are numpy arrays, after .to(device) `logp` and `nxt` are device tensors."""

    def __init__(self, logp, nxt, start, bos, eos, order, logp64=None):
        self.logp, self.nxt, self.start, self.bos, self.eos, self.order, self.logp64 = logp, nxt, int(start), int(bos), int(eos), \
            int(order), logp64
        self.S, self.V = int(logp.shape[0]), int(logp.shape[1])

    def to(self, device):
        import torch
        if isinstance(self.logp, torch.Tensor):
            return NgramTable(self.logp.to(device), self.nxt.to(device), self.start, self.bos, self.eos, self.order)
        return NgramTable(torch.from_numpy(np.ascontiguousarray(self.logp)).to(device),
                          torch.from_numpy(np.ascontiguousarray(self.nxt)).to(device), self.start, self.bos, self.eos, self.order)


class NgramLM(object):
    """prob: {n-gram (a tuple of ids): ln p(last | the others)}, backoff: {context tuple: ln backoff weight}."""

    def __init__(self, order, V, bos, eos, prob, backoff, oov_logp=-30.0):
        self.order, self.V, self.bos, self.eos = int(order), int(V), int(bos), int(eos)
        self.oov_logp = float(oov_logp)
        if not math.isfinite(self.oov_logp):
            raise ValueError("oov_logp must be finite, got %r" % (oov_logp,))
        if self.order < 1:
            raise ValueError("the order of an n-gram model is at least 1, got %d" % self.order)
        if not (0 < self.bos < self.V and 0 < self.eos < self.V and self.bos != self.eos):
            raise ValueError("<s> = %d and </s> = %d must be two ids in 1 .. V - 1 = %d (0 is the blank)" % (bos, eos, V - 1))
        self.prob = {tuple(int(i) for i in g): float(p) for g, p in prob.items()}
        self.backoff = {tuple(int(i) for i in g): float(b) for g, b in backoff.items()}
        for g in list(self.prob) + list(self.backoff):
            if len(g) > self.order or any(not 0 < i < self.V for i in g):
                raise ValueError("n-gram %r does not fit order %d over the ids 1 .. %d" % (g, self.order, self.V - 1))
        self._table = None
        self._device = {}

    # ------------------------------------------------------------------------------------------------------------ ARPA
    @classmethod
    def from_arpa(cls, path_or_text, vocab, bos, eos, oov_logp=-30.0, V=None):
        """path_or_text: a file name, or the file's text (anything with a newline in it).  vocab: {ARPA word: model id};
        <s> and </s> map to bos and eos.  ValueError for a word that is neither.  V: the model's vocabulary size (default:
        the greatest id of vocab + 1)."""
        text = path_or_text
        if "\n" not in text:
            with open(os.fspath(path_or_text), "r", encoding="utf-8") as f:
                text = f.read()
        words = dict(vocab)
        words["<s>"], words["</s>"] = int(bos), int(eos)
        V = max(int(i) for i in words.values()) + 1 if V is None else int(V)
        counts, prob, backoff, n, seen_data = {}, {}, {}, 0, False
        for raw in text.splitlines():
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                seen_data = True
                continue
            if line == "\\end\\":
                break
            if not seen_data:
                continue
            if line.startswith("ngram ") and n == 0:
                k, c = line[6:].split("=")
                counts[int(k)] = int(c)
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-7])
                continue
            if n == 0:
                raise ValueError("ARPA: %r before any \\N-grams: section" % line)
            f = line.split()
            if len(f) not in (n + 1, n + 2):
                raise ValueError("ARPA: a %d-gram line with %d fields: %r" % (n, len(f), line))
            for w in f[1:n + 1]:
                if w not in words:
                    raise ValueError("ARPA: the word %r is not in the vocabulary" % w)
            g = tuple(int(words[w]) for w in f[1:n + 1])
            p = float(f[0])
            if not (g == (int(bos),) and p <= ARPA_NO_PROB):         # (<s> is a context: only its backoff counts)
                prob[g] = p * LN10
            if len(f) == n + 2:
                backoff[g] = float(f[n + 1]) * LN10
        if not counts:
            raise ValueError("ARPA: no \\data\\ section")
        return cls(max(counts), V, bos, eos, prob, backoff, oov_logp=oov_logp)

    def to_arpa(self, symbols=None):
        """The model as ARPA text (log10, 17 significant digits).  symbols: {id: word}; an id without one is written as its
        number, <s> and </s> as themselves."""
        sym = dict(symbols or {})
        sym[self.bos], sym[self.eos] = "<s>", "</s>"
        name = lambda i: sym.get(i, str(i))                          # noqa: E731
        by_n = {n: [] for n in range(1, self.order + 1)}
        for g in set(self.prob) | {g for g in self.backoff if g}:
            by_n[len(g)].append(g)
        out = ["\\data\\"] + ["ngram %d=%d" % (n, len(by_n[n])) for n in range(1, self.order + 1)] + [""]
        for n in range(1, self.order + 1):
            out.append("\\%d-grams:" % n)
            for g in sorted(by_n[n]):
                p = self.prob[g] / LN10 if g in self.prob else ARPA_NO_PROB
                line = "%.17g\t%s" % (p, " ".join(name(i) for i in g))
                if g in self.backoff:
                    line += "\t%.17g" % (self.backoff[g] / LN10)
                out.append(line)
            out.append("")
        out.append("\\end\\")
        return "\n".join(out) + "\n"

    # ------------------------------------------------------------------------------------------------------- estimation
    @classmethod
    def estimate(cls, id_sequences, order, V, bos, eos, oov_logp=-30.0):
        """Interpolated Witten-Bell from lists of label ids: with N(h) the count of context h, T(h) its distinct successors,
            p(w | h) = (c(h w) + T(h) p(w | h')) / (N(h) + T(h)),   h' = h without its first token,
        down to p(w | empty context) interpolated with the uniform distribution over the events E = {1 .. V - 1} \\ {bos}
        (</s> among them), so that every event has a unigram.  Written in backoff form: a seen n-gram lists p(w | h), its
        context the backoff T(h) / (N(h) + T(h)) - for an unseen w that IS the interpolation.  Every context's
        distribution over E sums to 1."""
        order, V, bos, eos = int(order), int(V), int(bos), int(eos)
        events = [w for w in range(1, V) if w != bos]
        cnt = [dict() for _ in range(order)]                     # cnt[n][h] = {w: count}, len(h) = n
        for seq in id_sequences:
            toks = [bos] + [int(t) for t in seq] + [eos]
            for t in toks[1:-1]:
                if not (0 < t < V) or t in (bos, eos):
                    raise ValueError("estimate: label %d is not a label of 1 .. %d (<s> %d, </s> %d)" % (t, V - 1, bos, eos))
            for i in range(1, len(toks)):
                for n in range(order):
                    if i - n < 0:
                        break
                    d = cnt[n].setdefault(tuple(toks[i - n:i]), {})
                    d[toks[i]] = d.get(toks[i], 0) + 1
        prob, backoff = {}, {}
        uni = cnt[0].get((), {})
        N0, T0 = sum(uni.values()), len(uni)
        p_uni = {w: (uni.get(w, 0) + (T0 if T0 else 1) / len(events)) / (N0 + (T0 if T0 else 1)) for w in events}
        for w in events:
            prob[(w,)] = math.log(p_uni[w])
        interp = {(): p_uni}                                     # interp[h][w] for the SEEN w of h (all events for h = ())

        def p_of(h, w):                                          # interpolated p(w | h), h any context
            while True:
                d = interp.get(h)
                if d is not None and w in d:
                    return d[w] * 1.0
                if d is not None:                                # h seen, w not: the backoff mass times the lower order
                    return lam[h] * p_of(h[1:], w)
                h = h[1:]
        lam = {}
        for n in range(1, order):
            for h, d in cnt[n].items():
                N, T = sum(d.values()), len(d)
                lam[h] = T / (N + T)
                interp[h] = {}
            for h, d in cnt[n].items():
                N, T = sum(d.values()), len(d)
                for w, c in d.items():
                    interp[h][w] = (c + T * p_of(h[1:], w)) / (N + T)
                    prob[h + (w,)] = math.log(interp[h][w])
                backoff[h] = math.log(lam[h])
        return cls(order, V, bos, eos, prob, backoff, oov_logp=oov_logp)

    # ------------------------------------------------------------------------------------------------- host evaluation
    def token_logp(self, context, c):
        """ln p(c | context) by explicit backoff (float64): the longest listed n-gram that ends the context . c, plus the
        backoffs of the contexts given up on the way, summed in that order; oov_logp for a c without a unigram."""
        c = int(c)
        if (c,) not in self.prob:
            return self.oov_logp
        h = tuple(int(i) for i in context)[max(0, len(context) - (self.order - 1)):] if self.order > 1 else ()
        acc = 0.0
        while True:
            p = self.prob.get(h + (c,))
            if p is not None:
                return acc + p
            acc += self.backoff.get(h, 0.0)
            h = h[1:]

    def token_scores(self, ids, eos_term=True):
        """-> the float64 ln p of every token of ids given (<s>, the tokens before it), and of </s> behind them."""
        ctx, out = (self.bos,), []
        for c in list(ids) + ([self.eos] if eos_term else []):
            out.append(self.token_logp(ctx, c))
            ctx = ctx + (int(c),)
        return out

    def score(self, ids, eos_term=True):
        return float(sum(self.token_scores(ids, eos_term)))

    # -------------------------------------------------------------------------------------------------------- automaton
    def states(self):
        """The contexts that are states, in a fixed order: <s>, the empty context, then every context of length
        1 .. order - 1 that is the history of a listed n-gram or a listed n-gram below the top order, with their prefixes
        (sorted by length, then by ids)."""
        found = set()
        for g in self.prob:
            if 1 <= len(g) - 1 <= self.order - 1:
                found.add(g[:-1])
            if 1 <= len(g) <= self.order - 1:
                found.add(g)
        for g in self.backoff:
            if 1 <= len(g) <= self.order - 1:
                found.add(g)
        for g in list(found):                                    # (an ARPA file lists every prefix of what it lists; a model
            for n in range(1, len(g)):                           # given as dictionaries may not: the walk needs the prefixes)
                found.add(g[:n])
        found.discard((self.bos,))
        return [(self.bos,), ()] + sorted(found, key=lambda g: (len(g), g))

    def compile(self):
        """-> NgramTable, computed once.  Row `state`: logp[c] = token_logp(state, c) resolved in float64 (a row is the row
        of the state's longest proper suffix that is a state plus the state's backoff, the listed n-grams written over
        it) and rounded to float32 once; nxt[c] = the state of the longest suffix of state . c.  Validated here - the
        kernels trust the table: 0 <= nxt < S, S V < 2**31, every logp finite."""
        if self._table is not None:
            return self._table
        states = self.states()
        S, V = len(states), self.V
        if S * V >= 2 ** 31:
            raise ValueError("the automaton has %d states x %d tokens: S V must stay below 2**31" % (S, V))
        index = {s: i for i, s in enumerate(states)}
        children = {}
        for s, i in index.items():
            if len(s) >= 1:
                children.setdefault(s[:-1], []).append((s[-1], i))
        listed = {}
        for g, p in self.prob.items():
            listed.setdefault(g[:-1], []).append((g[-1], p))
        has_uni = np.zeros(V, dtype=bool)
        for g in self.prob:
            if len(g) == 1:
                has_uni[g[0]] = True
        logp = np.empty((S, V), dtype=np.float64)
        nxt = np.empty((S, V), dtype=np.int64)
        lim = self.order - 1
        order_of_rows = sorted(range(S), key=lambda i: (min(len(states[i]), lim), i))         # a row after its suffixes'
        for i in order_of_rows:
            s = states[i]
            h = s[max(0, len(s) - lim):] if lim > 0 else ()         # (order 1: <s> is a state that carries no context)
            if len(h) == 0:
                logp[i] = self.oov_logp
                nxt[i] = index[()]
            else:
                base = h[1:]
                while base not in index:
                    base = base[1:]
                logp[i] = logp[index[base]] + self.backoff.get(h, 0.0)
                nxt[i] = nxt[index[base]]
            for c, p in listed.get(h, ()):
                logp[i, c] = p
            # the successors: suffixes of h from the shortest to the longest, a longer one writes over a shorter one
            for j in range(len(h), -1, -1):
                sfx = h[j:]
                if len(sfx) + 1 > lim:
                    continue
                for c, k in children.get(sfx, ()):
                    nxt[i, c] = k
        logp[:, ~has_uni] = self.oov_logp
        logp[:, 0] = 0.0
        nxt[:, 0] = np.arange(S)
        if not np.isfinite(logp).all():
            raise ValueError("the automaton holds a log-probability that is not finite")
        if nxt.min() < 0 or nxt.max() >= S:
            raise ValueError("the automaton holds a successor outside 0 .. %d" % (S - 1))
        self._table = NgramTable(logp.astype(np.float32), nxt.astype(np.int32), index[(self.bos,)], self.bos, self.eos, self.order,
                                 logp64=logp)
        return self._table

    def to(self, device):
        """The compiled table on `device`, uploaded once per device."""
        key = str(device)
        if key not in self._device:
            self._device[key] = self.compile().to(device)
        return self._device[key]

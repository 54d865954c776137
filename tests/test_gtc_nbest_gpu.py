"""The device-side n-best graph builder (csrc/gtc_nbest.hip, ops.gtc_nbest_graphs) against its numpy reference
(tests/gtc_nbest_ref.py: the admission rule, gtc.nbest_weights, gtc.Graph.from_nbest, gtc._concat), the graph CTC loss on the
table it builds, and the Solver's pseudo-label step with `pseudo_graphs_on_gpu`.

Tolerances.  Every integer field, `start` and `dropped` are compared with torch.equal over the written extent.  The weights
are float64 on both sides with libm's exp / log / log1p on one and the device's on the other: `fin` (rounded to fp32 once)
and `log_weights` (rounded here) may differ from the reference rounded to fp32 by 1 fp32 ulp, -inf must be -inf.  The loss
cases use test_gtc_gpu's allowance (4 x the float32 restatement's error, floor 8 ulps) against float64, and torch.equal
against the host-built table of the same lists for every row whose `fin` agrees bit for bit.  Each case prints a
`gtc-nbest-parity` line (profiles/gtc_nbest_parity.txt holds one run)."""
import numpy as np
import pytest
import torch

import gtc_nbest_ref as NR
import gtc_ref as R
import poison as P
import test_gtc_gpu as TG

pytestmark = pytest.mark.gpu
DEV = "cuda"
NINF = -np.inf


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as entry
    entry.build()
    assert torch.cuda.is_available()
    import hip_backend
    return hip_backend


def _build(hyp, hyp_len, score, V, temperature=1.0):
    import ops
    return ops.gtc_nbest_graphs(torch.from_numpy(np.ascontiguousarray(hyp, dtype=np.int32)).to(DEV),
                                torch.from_numpy(np.ascontiguousarray(hyp_len, dtype=np.int32)).to(DEV),
                                torch.from_numpy(np.ascontiguousarray(score, dtype=np.float32)).to(DEV), V, temperature)


def _host(table):
    """The device table's arrays on the host, cut to their written extent (the test's own read: the operator makes none)."""
    out = {name: getattr(table, name).cpu() for name in table.FIELDS}
    NN = int(out["node_off"][-1])
    A = int(out["in_ptr"][NN])
    for name in ("lab", "start", "fin", "order"):
        out[name] = out[name][:NN]
    for name in ("in_ptr", "out_ptr"):
        out[name] = out[name][:NN + 1]
    for name in ("in_src", "in_w", "out_dst", "out_w"):
        out[name] = out[name][:A]
    out["graph_of"], out["dropped"], out["log_weights"] = table.graph_of.cpu(), table.dropped.cpu(), table.log_weights.cpu()
    return out


def _ulps(got, want, slack=0.0):
    """the largest distance in fp32 ulps of `want` between two float32 tensors whose -inf entries coincide; a distance of at
    most `slack` (absolute) counts as none"""
    got, want = got.float(), want.float()
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and not bool(torch.isnan(got).any())
    fin = ~torch.isinf(want)
    if not bool(fin.any()):
        return 0.0
    ulp = torch.from_numpy(np.spacing(np.abs(want[fin].numpy()).astype(np.float32)))
    d = (got[fin].double() - want[fin].double()).abs()
    return float((torch.where(d <= slack, torch.zeros_like(d), d) / ulp.double()).max())


def _compare(table, ref, what, slack=0.0):
    """The device table against the reference: -> the host copy.  Integers, start and the arc weights exactly; fin and
    log_weights within 1 fp32 ulp of the float64 reference rounded to fp32 (slack: see test_loss_through_the_table)."""
    got, want = _host(table), ref.table
    B = len(ref.graphs)
    assert torch.equal(got["node_off"], torch.from_numpy(want.node_off)), what
    assert torch.equal(got["graph_of"], torch.arange(B, dtype=torch.int32))
    for name in NR.INT_FIELDS + ("head", "start", "in_w", "out_w"):
        w = torch.from_numpy(np.ascontiguousarray(getattr(want, name)))
        assert got[name].shape == w.shape and torch.equal(got[name], w), "%s: %s" % (what, name)
    assert torch.equal(got["dropped"], torch.from_numpy(ref.dropped.astype(np.int32))), what
    u_fin = _ulps(got["fin"], torch.from_numpy(want.fin), slack)
    u_w = _ulps(got["log_weights"], torch.from_numpy(ref.log_weights.astype(np.float32)), slack)
    assert (table.max_nodes, table.max_arcs) == (table.cap_nodes, 3 * table.cap_nodes)
    assert max(g.N for g in ref.graphs) <= table.max_nodes and max(g.A for g in ref.graphs) <= table.max_arcs
    print("gtc-nbest-parity %s: %d rows, %d nodes, %d arcs (largest graph %d of %d), dropped %d, integers / start exact, fin "
          "%.2f ulp, log_weights %.2f ulp" % (what, B, int(got["node_off"][-1]), len(got["in_src"]),
                                               max(g.N for g in ref.graphs), table.max_nodes, int(ref.dropped.sum()), u_fin, u_w))
    assert u_fin <= 1.0 and u_w <= 1.0, what
    return got


def _pad(lists, K, L):
    """[(tokens or None: a dead slot, score)] per row -> hyp, hyp_len, score in the layout of ops.ctc_beam"""
    B = len(lists)
    hyp = np.full((B, K, L), -1, dtype=np.int32)
    hyp_len = np.full((B, K), -1, dtype=np.int32)
    score = np.full((B, K), NINF, dtype=np.float32)
    for b, row in enumerate(lists):
        for k, (h, s) in enumerate(row):
            if h is not None:
                hyp[b, k, :len(h)], hyp_len[b, k] = h, len(h)
            score[b, k] = s
    return hyp, hyp_len, score


HAND_V = 5
HAND = [
    [([1, 2, 3], -0.5), ([1, 2], -1.0), ([1, 2, 4, 4], -1.5), ([1, 3], -2.5)],       # shared prefixes, a prefix of another,
                                                                                     # a child with its parent's token
    [([2, 2, 1], -0.2), ([3], -0.9), ([2, 2, 1], -1.1), ([2], -3.0)],                # a duplicate pair
    [([], -0.1), ([1], -0.4), ([1, 1], -2.0), ([4, 3, 2, 1, 2, 3], -2.2)],           # the empty hypothesis live
    [([1, 2], -0.3), (None, NINF), ([3, 3, 3], NINF), ([1, 4], -0.8)],               # dead slots in the middle
    [(None, NINF), ([2, 1], NINF), (None, -1.0), (None, NINF)],                      # no live slot
    [(None, NINF), ([3, 3, 2], -7.5), (None, NINF), (None, NINF)],                   # a single live hypothesis
]


def _hand():
    return _pad(HAND, 4, 6)


# ------------------------------------------------------------------------------------------------ the table
def test_hand_made_lists(hb):
    hyp, hyp_len, score = _hand()
    for t in (1.0, 0.0):
        ref = NR.reference(hyp, hyp_len, score, HAND_V, t)
        assert [g.N for g in ref.graphs][4:] == [1, 7] and float(ref.graphs[5].fin[5]) == 0.0
        got = _compare(_build(hyp, hyp_len, score, HAND_V, t), ref, "hand-made B=6 K=4 L=6 V=5 t=%g" % t)
    n0 = int(got["node_off"][5])
    assert float(got["fin"][n0 + 5]) == 0.0 and float(got["fin"][n0 + 6]) == 0.0       # the single hypothesis weighs exactly 0
    assert float(got["fin"][int(got["node_off"][4])]) == 0.0


@pytest.mark.parametrize("temperature", [0.0, 0.7, 3.0])
def test_random_lists(hb, temperature):
    B, K, L, V = 8, 16, 40, 6
    hyp, hyp_len, score = NR.random_lists(np.random.RandomState(11), B, K, L, V, share=0.4)
    ref = NR.reference(hyp, hyp_len, score, V, temperature)
    assert not ref.dropped.any() and max(g.N for g in ref.graphs) > 2 * 256 + 1     # more trie nodes than threads
    _compare(_build(hyp, hyp_len, score, V, temperature), ref, "random B=8 K=16 L=40 V=6 t=%g" % temperature)


def _limit():
    rs = np.random.RandomState(17)
    K, L, V = 16, 65, 18
    hyp = rs.randint(1, V, size=(2, K, L)).astype(np.int32)
    hyp[:, :, 0] = np.arange(1, K + 1)                         # distinct first tokens: nothing is shared
    hyp_len = np.full((2, K), L, dtype=np.int32)
    hyp_len[1, K - 1] = NR.MAX_TRIE - (K - 1) * L             # row 1: exactly 1023 trie nodes
    hyp[1, K - 1, hyp_len[1, K - 1]:] = -1
    score = -np.sort(np.abs(rs.normal(0, 2, size=(2, K))), axis=1).astype(np.float32)
    return hyp, hyp_len, score, V


def test_the_node_limit(hb):
    """16 x 65 tokens with distinct first tokens are 1040 trie nodes, the smallest shape above 1023: the last slot is
    dropped and the weights renormalised; beside it a row at exactly 1023.  The loss on the table is finite."""
    import ops
    hyp, hyp_len, score, V = _limit()
    ref = NR.reference(hyp, hyp_len, score, V, 1.0)
    assert list(ref.dropped) == [1, 0] and [g.N for g in ref.graphs] == [2 * 15 * 65 + 1, 2047]
    table = _build(hyp, hyp_len, score, V, 1.0)
    got = _compare(table, ref, "limit K=16 L=65 (1040 and 1023 trie nodes)")
    N = got["node_off"][1:] - got["node_off"][:-1]
    assert int(N.max()) == hb.GTC_MAX_NODES == table.max_nodes
    assert bool(torch.isinf(got["log_weights"][0, 15])) and not bool(torch.isinf(got["log_weights"][1]).any())
    z = torch.from_numpy(np.random.RandomState(18).normal(0, 1, size=(2, 70, V)).astype(np.float32)).to(DEV).requires_grad_()
    nll = ops.gtc_loss(z, hb.to_device_i32([70, 68], DEV), table, False)
    nll.sum().backward()
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(z.grad).all())
    print("gtc-nbest-parity limit loss: nll %s finite on %d and %d nodes" % (nll.detach().cpu().tolist(), int(N[0]), int(N[1])))


# ------------------------------------------------------------------------------------------------ the loss through it
_LOSS = {}


def _loss_case():
    """The hand-made rows and four random ones (K = 4, L = 6) with their logits and the CPU results, computed once."""
    if _LOSS:
        return _LOSS
    rs = np.random.RandomState(23)
    V, T = HAND_V, 12
    hyp, hyp_len, score = _hand()
    h2, l2, s2 = NR.random_lists(rs, 4, 4, 6, V)
    hyp, hyp_len, score = np.concatenate([hyp, h2]), np.concatenate([hyp_len, l2]), np.concatenate([score, s2])
    B = len(hyp)
    ref = NR.reference(hyp, hyp_len, score, V, 0.7)
    lens = [T - (b % 4) for b in range(B)]
    z = torch.from_numpy(rs.normal(0, 1.5, size=(B, T, V)).astype(np.float32))
    for b, t in enumerate(lens):
        z[b, t:] = 0.0
    g = torch.from_numpy(rs.uniform(-2, 2, size=B).astype(np.float32))
    _LOSS.update(hyp=hyp, hyp_len=hyp_len, score=score, V=V, T=T, B=B, lens=lens, z=z, g=g, nbest=ref)
    _LOSS.update(TG._reference(z, lens, ref.graphs, g))
    assert bool(torch.isfinite(_LOSS["ref"][0]).all())
    return _LOSS


def _loss(hb, c, graphs, rows=None):
    import ops
    rows = list(range(c["B"])) if rows is None else rows
    z = c["z"][rows].to(DEV).requires_grad_()
    nll = ops.gtc_loss(z, hb.to_device_i32([c["lens"][i] for i in rows], DEV), graphs, True)
    nll.backward(c["g"][rows].to(DEV))
    return nll.detach().cpu(), z.grad.cpu()


def test_loss_through_the_table(hb):
    """nll and dlogits on the device table against float64 on the reference graphs, and against the host-built table.
    The table itself is compared here too, with one allowance the cases above do not need: row 9 holds the empty hypothesis
    three times, so its joined weight is log 1 - the reference gives -1.1e-16 and another libm +-1.1e-16 or 0, a distance
    that is nothing in float64 and has no measure in fp32 ulps of 0.  A distance of at most 32 x 2^-53 x (1 + max |t score|)
    - fewer than 32 float64 operations on numbers of that magnitude - counts as none; everything else stays at 1 fp32 ulp."""
    c = _loss_case()
    ref = c["nbest"]
    table = _build(c["hyp"], c["hyp_len"], c["score"], c["V"], 0.7)
    live = np.isfinite(c["score"])
    got = _compare(table, ref, "loss case B=10 K=4 L=6 V=5 t=0.7",
                   slack=32 * 2.0 ** -53 * (1.0 + 0.7 * float(np.abs(c["score"][live]).max())))
    nll, grad = _loss(hb, c, table)
    rows = torch.arange(c["B"])
    TG._check(c, nll, grad, rows, "gtc-nbest device table V=5")
    nll_h, grad_h = _loss(hb, c, ref.batch)                   # the host-built table of the same lists
    same = []
    for b in range(c["B"]):
        lo, hi = int(ref.table.node_off[b]), int(ref.table.node_off[b + 1])
        if torch.equal(got["fin"][lo:hi], torch.from_numpy(ref.table.fin[lo:hi])):
            same.append(b)
            assert torch.equal(nll[b], nll_h[b]) and torch.equal(grad[b], grad_h[b]), "row %d" % b
    assert 4 in same and 5 in same                             # no live slot / a single live hypothesis: weight exactly 0
    print("gtc-nbest-parity loss through the table: %d of %d rows with fin bit-equal to the host's, nll and dlogits bit-equal "
          "there (max_nodes %d against %d)" % (len(same), c["B"], table.max_nodes, ref.table.max_nodes))
    assert len(same) >= c["B"] // 2


# ------------------------------------------------------------------------------------------------ undefined memory
def _written(got):
    return [got[name] for name in sorted(got)]


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_undefined_memory(hb, pattern):
    """The table's arrays, the counts, nll, dlogits and the workspaces come from torch.empty: filled with the pattern, and
    taken from what a larger call left behind, the written extent, nll and dlogits have the bits of the clean run."""
    c = _loss_case()
    args = (c["hyp"], c["hyp_len"], c["score"], c["V"], 0.7)
    P.empty_pool()
    try:
        table = _build(*args)
        want = _written(_host(table)) + list(_loss(hb, c, table))
        for variant in ("fresh", "leftover"):
            st = P.Stats()
            P.empty_pool()
            if variant == "leftover":
                big = NR.random_lists(np.random.RandomState(29), 12, 8, 9, c["V"])
                bt = _build(*big, c["V"], 1.0)
                zb = torch.randn(12, c["T"], c["V"], device=DEV, requires_grad=True)
                import ops
                ops.gtc_loss(zb, hb.to_device_i32([c["T"]] * 12, DEV), bt, True).sum().backward()
                del bt, zb
                P.poison_pool(pattern, st)
            with P.poisoned(pattern, st):
                table = _build(*args)
                got = _written(_host(table)) + list(_loss(hb, c, table))
            assert st.total > 0
            for a, b in zip(got, want):
                assert torch.equal(a, b), (variant, pattern)
    finally:
        P.empty_pool()
    print("gtc-nbest-parity undefined memory %s: table, nll, dlogits bit-identical (fresh and leftover)" % pattern)


# ------------------------------------------------------------------------------------------------ batch independence
def _row_view(got, b):
    n0, n1 = int(got["node_off"][b]), int(got["node_off"][b + 1])
    a0, a1 = int(got["in_ptr"][n0]), int(got["in_ptr"][n1])
    assert int(got["out_ptr"][n0]) == a0 and int(got["out_ptr"][n1]) == a1
    return [got["lab"][n0:n1], got["start"][n0:n1], got["fin"][n0:n1], got["order"][n0:n1], got["head"][b],
            got["in_ptr"][n0:n1 + 1] - a0, got["out_ptr"][n0:n1 + 1] - a0, got["in_src"][a0:a1], got["out_dst"][a0:a1],
            got["in_w"][a0:a1], got["out_w"][a0:a1], got["dropped"][b], got["log_weights"][b]]


def test_batch_independence(hb):
    """A row alone, moved to another index, and beside other rows: its graph relative to its offsets, its weights and its
    nll and dlogits bits are the same."""
    c = _loss_case()
    B = c["B"]

    def run(rows):
        table = _build(c["hyp"][rows], c["hyp_len"][rows], c["score"][rows], c["V"], 0.7)
        got = _host(table)
        return [_row_view(got, r) for r in range(len(rows))], _loss(hb, c, table, rows)
    views, (nll, grad) = run(list(range(B)))
    rev = list(range(B))[::-1]
    views_r, (nll_r, grad_r) = run(rev)
    for r, i in enumerate(rev):
        assert all(torch.equal(a, b) for a, b in zip(views_r[r], views[i])), "moved: row %d" % i
        assert torch.equal(nll_r[r], nll[i]) and torch.equal(grad_r[r], grad[i]), "moved: row %d" % i
    for i in range(B):
        v1, (n1, g1) = run([i])
        assert all(torch.equal(a, b) for a, b in zip(v1[0], views[i])), "alone: row %d" % i
        assert torch.equal(n1[0], nll[i]) and torch.equal(g1[0], grad[i]), "alone: row %d" % i
    some = [7, 2, 5]
    v3, (n3, g3) = run(some)
    for r, i in enumerate(some):
        assert all(torch.equal(a, b) for a, b in zip(v3[r], views[i])) and torch.equal(n3[r], nll[i]) and torch.equal(g3[r], grad[i])
    print("gtc-nbest-parity batch independence: %d rows alone, moved, beside other rows: graph, weights, nll, dlogits "
          "bit-identical" % B)


# ------------------------------------------------------------------------------------------------ the Solver
class _NoHostRead(object):
    """No device-to-host copy inside the scope: torch.cuda.set_sync_debug_mode("error") where torch honours it (probed with
    an .item() first), and Tensor.cpu / .item / .tolist raising either way.  leave() ends it (idempotent)."""

    def __init__(self):
        self.on, self.saved, self.used = False, {}, None

    def enter(self):
        probe = torch.ones(1, device=DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if not honoured:
            torch.cuda.set_sync_debug_mode("default")
        self.used = 'set_sync_debug_mode("error") and raising Tensor.cpu/.item/.tolist' if honoured else \
            "raising Tensor.cpu/.item/.tolist (set_sync_debug_mode is not honoured)"

        def refuse(name):
            def raising(*a, **k):
                raise AssertionError("Tensor.%s between the entry of the pseudo-label step and _step" % name)
            return raising
        for name in ("cpu", "item", "tolist"):
            self.saved[name] = getattr(torch.Tensor, name)
            setattr(torch.Tensor, name, refuse(name))
        self.on = True

    def leave(self):
        if self.on:
            torch.cuda.set_sync_debug_mode("default")
            for name, f in self.saved.items():
                setattr(torch.Tensor, name, f)
            self.on = False


def test_solver_step_on_the_device(hb, tmp_path, monkeypatch):
    """test_gtc_gpu.test_pseudo_train_step with `pseudo_graphs_on_gpu`: the loss is composed from the device list exactly as
    there (pseudo_weight x the mean of -logsumexp_k (log w_k - ops.ctc_loss of hypothesis k), within 32 fp32 ulps of the
    largest nll involved), the parameters move, one gtc_loss and one gtc_loss_bwd run, and nothing is read back between
    the entry and _step."""
    import ops
    K, weight, temp = 4, 0.5, 0.7
    solver, dev = TG._solver(str(tmp_path / "s"), monkeypatch, ctc_weight=0.3, deterministic=True, pseudo_beam=K,
                             pseudo_weight=weight, pseudo_temperature=temp, pseudo_graphs_on_gpu=True)
    xs, ilens, _ = TG._sup_batch(dev)
    net = solver.model
    B = len(ilens)
    with hb.deterministic():
        net.eval()
        hyp, hyp_len, score = net.ctc_beams_on_device(xs, ilens, K)
        net.train()
        table = ops.gtc_nbest_graphs(hyp, hyp_len, score, net.ctc_lo.out_features, temp)
        h_hyp, h_len, logw = hyp.cpu().numpy(), hyp_len.cpu().numpy(), table.log_weights.cpu().numpy()
        assert int(table.dropped.sum()) == 0 and bool((h_len[:, 0] >= 0).all())
        with torch.no_grad():
            enc_h, _ = net.encoder(xs, ilens)
            logits = ops.linear(enc_h.reshape(-1, enc_h.shape[2]), net.ctc_lo.weight, net.ctc_lo.bias).view(B, enc_h.shape[1], -1)
            rows, top = [], 0.0
            for b in range(B):
                terms = []
                for k in range(K):
                    if h_len[b, k] < 0 or logw[b, k] == NINF:
                        continue
                    h = [int(v) for v in h_hyp[b, k, :h_len[b, k]]]
                    nk = ops.ctc_loss(logits[b:b + 1], net.encoder.enc2.last_lens_dev[b:b + 1],
                                      torch.tensor(h if h else [1], dtype=torch.long, device=dev)[:len(h)], [len(h)], False)
                    terms.append(float(logw[b, k]) - float(nk))
                    top = max(top, abs(float(nk)))
                rows.append(-float(torch.logsumexp(torch.tensor(terms, dtype=torch.float64), 0)))
        want = weight * sum(rows) / B
        before = {n: p.detach().clone() for n, p in net.named_parameters()}
        guard, inner = _NoHostRead(), solver._step

        def step(*a, **k):
            guard.leave()                                      # the window ends where _step begins
            return inner(*a, **k)
        monkeypatch.setattr(solver, "_step", step)
        torch.cuda.synchronize()
        launches = dict(hb.LAUNCHES)
        guard.enter()
        try:
            loss, mean = solver.pseudo_train_one_iteration(xs, ilens)
        finally:
            guard.leave()
        solver.flush()
    last = solver.last_pseudo
    assert last["graphs"].__class__.__name__ == "DeviceGraphTable" and all(last[k].is_cuda for k in ("hyp", "hyp_len", "score",
                                                                                                     "log_weights", "dropped"))
    assert torch.equal(last["hyp_len"], hyp_len) and torch.equal(last["score"], score)
    assert torch.equal(last["log_weights"], table.log_weights)
    assert torch.equal(torch.where(last["hyp_len"].unsqueeze(2) > torch.arange(hyp.shape[2], device=dev), last["hyp"], -1),
                       torch.where(hyp_len.unsqueeze(2) > torch.arange(hyp.shape[2], device=dev), hyp, -1))
    delta = {k: v - launches.get(k, 0) for k, v in hb.LAUNCHES.items() if v != launches.get(k, 0)}
    assert delta.get("gtc_loss") == 1 and delta.get("gtc_loss_bwd") == 1 and delta.get("gtc_nbest") == 1
    print("gtc-nbest-parity solver step on the device: loss %.7f, composed %.7f, largest nll %.4g; no host read before _step by "
          "%s" % (float(loss), want, top, guard.used))
    assert np.isfinite(float(loss)) and abs(float(loss) - weight * float(mean)) <= 4 * 2.0 ** -23 * abs(float(loss))
    assert abs(float(loss) - want) <= 32 * 2.0 ** -23 * max(top, abs(want))
    moved = [n for n, p in net.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert "ctc_lo.weight" in moved and any(n.startswith("encoder.") for n in moved)
    assert not hb.persist_aborted(dev)


def test_solver_key_off_is_the_host_path(hb, tmp_path, monkeypatch):
    """Without the key and with it false the pseudo-label step is the same step: the same launches - none of the builder -
    and the same loss bits (deterministic mode)."""
    seen = []
    for run, over in enumerate((dict(), dict(pseudo_graphs_on_gpu=False))):
        solver, dev = TG._solver(str(tmp_path / ("run%d" % run)), monkeypatch, ctc_weight=0.3, deterministic=True, pseudo_beam=4,
                                 pseudo_weight=0.5, pseudo_temperature=0.7, **over)
        hb.persist_clear_abort(dev)
        xs, ilens, _ = TG._sup_batch(dev)
        before = dict(hb.LAUNCHES)
        with hb.deterministic():
            loss, _ = solver.pseudo_train_one_iteration(xs, ilens)
            solver.flush()
        delta = {k: v - before.get(k, 0) for k, v in hb.LAUNCHES.items() if v != before.get(k, 0)}
        assert "ids" in solver.last_pseudo and solver.last_pseudo["graphs"].__class__.__name__ == "GraphBatch"
        seen.append((delta, np.float32(float(loss))))
    assert seen[0][0] == seen[1][0] and "gtc_nbest" not in seen[0][0]
    assert seen[0][0].get("gtc_loss") == 1 and seen[0][0].get("gtc_loss_bwd") == 1
    assert seen[0][1].tobytes() == seen[1][1].tobytes()
    print("gtc-nbest-parity solver key off: launches and loss bits of the host path, no builder launch")

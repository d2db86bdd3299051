"""-m gpu: the one-launch score product + candidate reduction (torch.ops.gnnpn.score_select, csrc/score_select.hip) against the
two launches it replaces — torch.ops.gnnpn.linear(..., ACT_SIGMOID) followed by segment_topk_feasible — with torch.equal on all
three outputs (scores, pn-input rows, candidate ids).

One table holds categories of 1, 15, 16, 17, 53, 64 and 256 services (256 = score_plan.MAX_CATEGORY, the kernel's cap); the
category of 53 lies across column 64 of the old GEMM's tiles and the one of 256 across 192, 256, 320 and 384.  B = 17: a full
tile of 16 problems and a tile of one.  Per (problem, category) the bounds are wide open, a narrow cost window (fewer feasible
services than n_per: cyclic repetition), empty (dummy rows, -1 ids), or the category is absent.  Ties come from duplicated
service-embedding rows (bit-equal scores whatever the product does), and from rows whose product is so negative for every problem
that the sigmoid gives +0.0 for different services; the reference's own rule (lowest id) decides both.  A -0.0 score cannot be
produced: both paths form the scores themselves and 1 / (1 + exp(-v)) is never negative — the zero canonicalisation of
rank_key is the same function in both kernels (csrc/select_keys.h) and is tested on given scores in test_gpu_abi_layout.py.

A second, small table (categories of 65, 100, 128 and 3 services) runs the size class of 8 keys per lane, which the first table's
categories skip, and is held to the rule written out on the CPU as well: both launches now share the rule's code (select_keys.h).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 53, 64, 256)
B, K = 17, 128
N_PER = (1, 5, 16)
ZERO_ROWS = (180, 181, 300)            # services of the last category whose score is +0.0 for every problem
DUPLICATES = ((49, 50), (55, 60), (55, 61), (170, 200), (170, 421), (16, 31), (1, 15))


def _inputs():
    from gnnpn_sc_amd import score_plan
    assert max(SIZES) == score_plan.MAX_CATEGORY
    g = torch.Generator().manual_seed(9)
    cat = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    S, T = int(cat[-1]), len(SIZES)
    xr = torch.randn(B, K, generator=g)
    xr[:, 0] = 8.0
    emb = torch.randn(S, K, generator=g) * 0.1
    for src, dst in DUPLICATES:
        emb[dst] = emb[src]
    for s in ZERO_ROWS:
        emb[s, 0] = -40.0                                  # product about -320: exp(320) overflows, the sigmoid is +0.0
    qos = torch.rand(S, 4, generator=g, dtype=torch.float64)
    for i, s in enumerate(ZERO_ROWS):
        qos[s, 2] = 0.5 + 1e-4 * i
    others = torch.ones(S, dtype=torch.bool)
    others[list(ZERO_ROWS)] = False
    near = others & (qos[:, 2] > 0.4998) & (qos[:, 2] < 0.5004) & (torch.arange(S) >= int(cat[-2]))
    qos[near, 2] = 0.6                                     # nobody else of that category inside the zero rows' window
    lb = torch.empty(B, T, 4, dtype=torch.float64)
    present = torch.ones(B, T, dtype=torch.uint8)
    for b in range(B):
        for c in range(T):
            mode = (b + 2 * c) % 5
            lo = float(torch.rand((), generator=g)) * 0.8
            if mode == 0:
                lb[b, c] = torch.tensor([0.0, 1.0, 0.0, 1.0])
            elif mode == 1:
                lb[b, c] = torch.tensor([lo, lo + 0.08, 0.0, 1.0])
            elif mode == 2:
                lb[b, c] = torch.tensor([0.7, 0.3, 0.0, 1.0])          # nothing feasible
            elif mode == 3:
                lb[b, c] = torch.tensor([0.0, 1.0, 0.0, 1.0])
                present[b, c] = 0
            else:
                lb[b, c] = torch.tensor([lo, lo + 0.3, 0.1, 0.9])
    for b in (0, 5, 16):                                   # only the +0.0 services of the last category are feasible
        lb[b, T - 1] = torch.tensor([0.49999, 0.50025, 0.0, 1.0])
        present[b, T - 1] = 1
    gb = torch.rand(B, 4, generator=g, dtype=torch.float64)
    return {"cat": cat, "xr": xr, "emb": emb, "qos": qos, "lb": lb, "present": present, "gb": gb, "S": S, "T": T}


@pytest.fixture(scope="module")
def case(dev):
    """The inputs on the device and the two-launch reference for every n_per, computed once."""
    from gnnpn_sc_amd import custom_ops, ops   # noqa: F401
    h = _inputs()
    d = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(dev) for k, v in h.items() if k not in ("S", "T")}
    scores = torch.ops.gnnpn.linear(d["xr"], d["emb"], act=ops.ACT_SIGMOID)
    ref = {n: (scores, *torch.ops.gnnpn.segment_topk_feasible(scores, d["cat"], d["qos"], d["lb"], d["present"], d["gb"], n)) for n in N_PER}
    torch.cuda.synchronize()
    return h, d, ref


def test_the_reference_holds_the_cases(case):
    """What the comparison below is worth: the reference itself shows dummy rows, cyclic repetition, bit-equal positive ties, +0.0
    ties decided by the lowest id, and an absent category."""
    h, d, ref = case
    scores = ref[5][0].cpu()
    for src, dst in DUPLICATES:
        assert torch.equal(scores[:, src], scores[:, dst])
    z = scores[:, list(ZERO_ROWS)]
    assert (z == 0).all() and not torch.signbit(z).any()
    ids = ref[5][2].cpu().view(B, h["T"], 5)
    assert (ids[h["present"] == 0] == -1).all() and int((h["present"] == 0).sum()) > 0
    dummy = (ids == -1).all(-1) & (h["present"] == 1)
    assert int(dummy.sum()) > 0
    found = ids[..., 0] >= 0
    distinct = torch.tensor([[len(set(ids[b, c].tolist())) for c in range(h["T"])] for b in range(B)])
    big = torch.tensor(SIZES) >= 5
    assert int((found & (distinct < 5) & big[None, :]).sum()) > 0                      # fewer feasible than n_per in a category that has 5
    for b in (0, 5, 16):
        assert ids[b, h["T"] - 1].tolist() == [180, 181, 300, 180, 181]                # +0.0 ties: lowest id first, then cyclic


@pytest.mark.parametrize("n_chunks", [2, 3, 12])
@pytest.mark.parametrize("n_per", N_PER)
def test_score_select_equals_linear_then_select(case, n_per, n_chunks):
    """Two chunks (six categories in 13 tiles, and the category of 256 in 16), three (fewer chunks than categories, one of them
    empty) and twelve (more chunks than categories): the same bits as the two launches in every output."""
    from gnnpn_sc_amd import score_plan
    h, d, ref = case
    plan = score_plan.plan_chunks(h["cat"], n_chunks)
    assert plan is not None and plan.n_chunks == n_chunks and plan.fits()
    assert (n_chunks < h["T"]) == (n_chunks in (2, 3))
    packed = score_plan.pack_embedding(d["emb"], plan)
    plan_host, plan_dev = plan.tensors(d["emb"].device)
    for _ in range(2):                                     # a second call: nothing is left behind by the first
        scores, rows, ids = torch.ops.gnnpn.score_select(d["xr"], packed, plan_host, plan_dev, d["qos"], d["lb"], d["present"], d["gb"], n_per)
        want = ref[n_per]
        assert torch.equal(scores, want[0])
        assert torch.equal(ids, want[2])
        assert torch.equal(rows, want[1])


def test_a_plan_the_kernel_cannot_hold_is_refused(case):
    """The host copy of the plan is checked before the launch: a chunk of more tiles than a workgroup holds, and a plan whose
    pointers do not end at T, raise."""
    from gnnpn_sc_amd import score_plan
    h, d, ref = case
    cat2 = np.concatenate([h["cat"], h["cat"][1:] + h["S"]]).astype(np.int32)           # 58 tiles in one chunk
    bad = score_plan.ScorePlan(cat2, np.array([0, len(cat2) - 1]))
    assert not bad.fits()
    emb2 = torch.cat([d["emb"], d["emb"]])
    args = (torch.cat([d["qos"], d["qos"]]), torch.cat([d["lb"], d["lb"]], 1), torch.cat([d["present"], d["present"]], 1), d["gb"], 5)
    with pytest.raises(RuntimeError, match="a workgroup holds"):
        torch.ops.gnnpn.score_select(d["xr"], score_plan.pack_embedding(emb2, bad), *bad.tensors(emb2.device), *args)
    plan = score_plan.plan_chunks(h["cat"], 3)
    host, devp = plan.tensors(d["emb"].device)
    host = host.clone()
    host[4 + 2 * (plan.n_categories + 1) + plan.n_chunks] -= 1                     # chunk_ptr's last entry: no longer T
    with pytest.raises(RuntimeError, match="do not span"):
        torch.ops.gnnpn.score_select(d["xr"], score_plan.pack_embedding(d["emb"], plan), host, devp, d["qos"], d["lb"], d["present"], d["gb"], 5)


def test_shape_outside_the_fused_conditions_takes_the_two_launches(dev):
    """Through the pipeline's own call: categories of 5 services on average and hidden size 64 — the fused kernel does not apply
    (no operands are made), and ``front`` returns what ``scores`` then ``candidates`` return."""
    import gnnpn_sc_amd.synth as synth
    from gnnpn_sc_amd.modelML import Net
    from gnnpn_sc_amd.modelPN import CombinatorialRL, reward
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices, ML2PNPipeline
    from oracle import ml as oml
    T, S, n_per, Bp, H = 12, 60, 3, 9, 32
    table = synth.make_service_table(T, S, seed=3, degree=4)
    pb = synth.make_problem_batch(table, Bp, seed=4, tasks_per_problem=5, lo_range=(0.85, 0.96))
    net = Net(64, S, 20, 2, 2)
    net.load_state_dict(oml.make_state_dict(64, 20, 2, 2, seed=5))
    low = CombinatorialRL(0, H, T * n_per, 0, 10, 1, reward, "Dot", n_per, T, level="Low")
    high = CombinatorialRL(0, H, T * n_per, 0, 10, 1, reward, "Dot", n_per, T, level="High")
    pipe = ML2PNPipeline(net.to(dev).eval(), low.to(dev).eval(), high.to(dev).eval(), n_per, precision="f32")
    svc, batch = DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev)
    assert pipe.score_select_operands(svc, batch) is None
    scores, rows, ids = pipe.front(svc, batch)
    want = pipe.scores(svc, batch)
    want_rows, want_ids = pipe.candidates(svc, batch, want)
    assert scores.shape == (Bp, S) and torch.equal(scores, want) and torch.equal(rows, want_rows) and torch.equal(ids, want_ids)


# ---- a second, small table: categories of 65, 100 and 128 services hold 5, 7 and 8 keys per lane, the size class of 8 that the
# table above (1, 1, 1, 2, 4, 4 and 16 keys) never reaches; 21 tiles and 4 categories, so ONE chunk holds them all
SIZES8 = (65, 100, 128, 3)
B8, N_PER8 = 3, (1, 16)
# (lower, upper) service ids with the same embedding row; in-category positions (10, 64), (5, 70), (80, 99), (63, 127), (64, 100):
# the upper one always in a key slot j >= 4, the lower one of three pairs below position 64.  The first pair scores highest in
# category 0 and service 165 + 90 (unduplicated, position 90) highest in category 2: what n_per = 1 picks in the open cells
DUPLICATES8 = ((10, 64), (70, 135), (145, 164), (228, 292), (229, 265))
TOP8 = 165 + 90
# per (problem, category): "open", a cost window of that many services, 0 = an empty window, None = the category is absent
CELLS8 = (("open", 9, 0, "open"), (15, "open", 1, None), (0, 4, "open", 2))


def _inputs8():
    g = torch.Generator().manual_seed(11)
    cat = np.concatenate([[0], np.cumsum(SIZES8)]).astype(np.int32)
    S, T = int(cat[-1]), len(SIZES8)
    xr = torch.randn(B8, K, generator=g)
    xr[:, 0] = 8.0
    emb = torch.randn(S, K, generator=g) * 0.1
    emb[DUPLICATES8[0][0], 0] = 1.0                        # + 8 in the product: above everything else of its category
    emb[TOP8, 0] = 1.0
    for src, dst in DUPLICATES8:
        emb[dst] = emb[src]
    qos = torch.rand(S, 4, generator=g, dtype=torch.float64)
    lb = torch.empty(B8, T, 4, dtype=torch.float64)
    present = torch.ones(B8, T, dtype=torch.uint8)
    for b in range(B8):
        for c in range(T):
            cell = CELLS8[b][c]
            cost = qos[int(cat[c]):int(cat[c + 1]), 2].sort().values
            if cell == "open" or cell is None:
                lb[b, c] = torch.tensor([0.0, 1.0, 0.0, 1.0])
                present[b, c] = 0 if cell is None else 1
            elif cell == 0:
                lb[b, c] = torch.tensor([0.7, 0.3, 0.0, 1.0])
            else:                                          # exactly `cell` services inside: the costs are distinct doubles
                first = (b + c) % (len(cost) - cell + 1)
                lb[b, c] = torch.tensor([float(cost[first]), float(cost[first + cell - 1]), 0.0, 1.0], dtype=torch.float64)
    gb = torch.rand(B8, 4, generator=g, dtype=torch.float64)
    return {"cat": cat, "xr": xr, "emb": emb, "qos": qos, "lb": lb, "present": present, "gb": gb, "S": S, "T": T}


def _cpu_picks(scores, h, n_per):
    """The rule itself, from given scores: per cell the feasible services by (score descending, -0 = +0; id ascending), the first
    n_per repeated cyclically, -1 and the dummy row where there is none; the global bounds behind category 0's rows.  Returns
    rows [B, T * n_per, 8], ids [B, T * n_per], the number of feasible services [B, T] and the distinct picks per cell."""
    cat, qos, lb, present, gb = h["cat"], h["qos"].numpy(), h["lb"].numpy(), h["present"].numpy(), h["gb"].numpy()
    nb, T = present.shape
    rows = np.zeros((nb, T, n_per, 8), np.float32)
    ids = np.full((nb, T, n_per), -1, np.int32)
    n_feasible = np.zeros((nb, T), np.int64)
    picked = {}
    for b in range(nb):
        for c in range(T):
            s = np.arange(cat[c], cat[c + 1])
            lo_c, hi_c, lo_q, hi_q = lb[b, c]
            ok = (present[b, c] != 0) & (lo_c <= qos[s, 2]) & (qos[s, 2] <= hi_c) & (lo_q <= qos[s, 3]) & (qos[s, 3] <= hi_q)
            f = s[ok]
            order = f[np.lexsort((f, -(scores[b, f] + np.float32(0.0))))]
            n_feasible[b, c], picked[b, c] = len(f), order[:n_per]
            rows[b, c, :, :4] = (0.0, 1.0, 1.0, 1.0)
            if len(order):
                ids[b, c] = order[:n_per][np.arange(n_per) % min(n_per, len(order))]
                rows[b, c, :, :4] = qos[ids[b, c]].astype(np.float32)
            if c == 0:
                rows[b, c, :, 4:] = gb[b].astype(np.float32)
    return rows.reshape(nb, T * n_per, 8), ids.reshape(nb, T * n_per), n_feasible, picked


@pytest.fixture(scope="module")
def case8(dev):
    from gnnpn_sc_amd import custom_ops, ops   # noqa: F401
    h = _inputs8()
    d = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(dev) for k, v in h.items() if k not in ("S", "T")}
    scores = torch.ops.gnnpn.linear(d["xr"], d["emb"], act=ops.ACT_SIGMOID)
    ref = {n: (scores, *torch.ops.gnnpn.segment_topk_feasible(scores, d["cat"], d["qos"], d["lb"], d["present"], d["gb"], n)) for n in N_PER8}
    torch.cuda.synchronize()
    return h, d, ref


@pytest.mark.parametrize("n_chunks", [1, 4])
@pytest.mark.parametrize("n_per", N_PER8)
def test_categories_of_five_to_eight_keys_per_lane(case8, n_per, n_chunks):
    """Categories of 65, 100 and 128 services (and one of 3) in one chunk and in one chunk each, B = 3 (one ragged tile of problems):
    the same bits as the two launches, and the same picks and rows as the rule written out on the CPU from the returned scores.
    Before either comparison the CPU side shows that the case holds what it is for: a cell without a feasible service, one with
    fewer than 16, a pick at an in-category position >= 64 and a tie decided between positions on both sides of 64."""
    from gnnpn_sc_amd import score_plan
    h, d, ref = case8
    assert [(n + 15) // 16 for n in SIZES8] == [5, 7, 8, 1]
    plan = score_plan.plan_chunks(h["cat"], n_chunks)
    assert plan is not None and plan.n_chunks == n_chunks and plan.fits() and score_plan.applies(h["cat"], K, n_per)
    packed = score_plan.pack_embedding(d["emb"], plan)
    plan_host, plan_dev = plan.tensors(d["emb"].device)
    scores, rows, ids = torch.ops.gnnpn.score_select(d["xr"], packed, plan_host, plan_dev, d["qos"], d["lb"], d["present"], d["gb"], n_per)

    want_rows, want_ids, n_feasible, picked = _cpu_picks(scores.cpu().numpy(), h, n_per)
    cat = h["cat"]
    for b in range(B8):
        for c in range(h["T"]):
            cell = CELLS8[b][c]
            assert n_feasible[b, c] == (SIZES8[c] if cell == "open" else 0 if cell is None else cell)
    assert int((n_feasible[h["present"].numpy() != 0] == 0).sum()) > 0 and int(((n_feasible > 0) & (n_feasible < 16)).sum()) > 0
    assert any(int(s) - int(cat[c]) >= 64 for (b, c), p in picked.items() for s in p)
    sc = scores.cpu().numpy()
    decided = [(b, lo, hi) for (b, c), p in picked.items() for lo, hi in DUPLICATES8
               if lo in p and lo - cat[c] < 64 <= hi - cat[c] < SIZES8[c] and n_feasible[b, c] == SIZES8[c] and sc[b, lo] == sc[b, hi]]
    assert decided                                         # both feasible (an open cell), equal scores, the lower id among the picks

    want = ref[n_per]
    assert torch.equal(scores, want[0])
    assert torch.equal(ids, want[2])
    assert torch.equal(rows, want[1])
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(rows.cpu().numpy(), want_rows)

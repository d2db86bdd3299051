"""Problems with repeated categories for the candidate-table builder (gnnpn_woa_candidates_count / _fill), host only and
deterministic from a seed: up to 200 task nodes over 40 categories, so that a problem has more than 64 — and more than 128 —
non-empty candidate lists with empty ones between them, action rows whose count is independent of the category count, and
what the host path (loadDataOther + WOA._prepare) says of them.  synth.make_problem_batch gives a problem one task per category
at the most; these problems exist here alone.  tests/test_candidate_tables_host.py holds the conditions the GPU tests rely on."""
import functools

import numpy as np

N_CAT, N_SERVICES = 40, 400
TASK_COUNTS = (1, 3, 63, 64, 65, 127, 128, 129, 130, 200)            # the sizes around the 64-slot passes of the kernels
MORE_COUNTS = (2, 5, 10, 20, 40, 66, 96, 131, 150, 160, 190, 200)
ALL_INFEASIBLE = (70, 3)                                              # problems without a single list: "no categories"
SEARCH_COUNTS = (3, 63, 65, 100, 130, 200)                            # the smaller batch the searches run on
REDUCTS = (0, 0.55, 0.3137)                                           # the last one: the "further drawn value" of the GPU tests
A_TS = (65, 130, 200)
SEED, SEARCH_SEED = 7, 8
NEVER = float(np.nextafter(np.float32(1.0), np.float32(0.0)))         # a lower bound inside [0.9, 1) that no service reaches
STATUS_OK, STATUS_ROWS_MISMATCH, STATUS_NO_SLOTS = 0, 1, 3


def _node(n_cat, index, floats):
    onehot = [0] * (n_cat + 1)
    onehot[index] = 1
    return onehot + [float(v) for v in floats]


def _chain(n_nodes):
    i = np.arange(n_nodes - 1)
    return [np.stack([i, i + 1], 1).reshape(-1).tolist(), np.stack([i + 1, i], 1).reshape(-1).tolist()]


def _problem(g, n_t, table, infeasible):
    """The request node, then n_t task nodes: categories drawn with replacement, lower bounds 0.9 + 0.1 u^2 (float32, widened), about
    one node in ten (``infeasible`` = 1: every node) with bounds no service meets.  The last node of a category sets its bounds."""
    from gnnpn_sc_amd.synth import REQUEST_FLOATS
    nodes = [_node(table.n_cat, 0, REQUEST_FLOATS)]
    cats = g.integers(0, table.n_cat, n_t)
    lo = (0.9 + 0.1 * g.random((n_t, 2)) ** 2).astype(np.float32).astype(np.float64)
    lo[g.random(n_t) < infeasible] = NEVER
    for c, (l0, l1) in zip(cats, lo):
        nodes.append(_node(table.n_cat, int(c) + 1, (1.0, l0, 1.0, 1.0, l1, 1.0)))
    return nodes


@functools.lru_cache(maxsize=None)
def make_dataset(seed=SEED, counts=TASK_COUNTS + MORE_COUNTS, all_infeasible=ALL_INFEASIBLE):
    """The five artefacts of synth.make_dataset.  The test quarter (the last one, which loadDataOther and tables_from_dataset read):
    one problem per entry of ``counts`` in a seeded order, the ``all_infeasible`` ones behind its first third and its second third —
    failed problems in the middle of the batch; the other three quarters: one task node each."""
    import gnnpn_sc_amd.synth as synth
    table = synth.make_service_table(N_CAT, N_SERVICES, seed, graph="none")
    assert float(table.qos[:, 2:].max()) < NEVER
    g = np.random.default_rng(seed + 1)
    order = [int(counts[i]) for i in g.permutation(len(counts))]
    spec = [(n, 0.1) for n in order]
    for k, n in enumerate(all_infeasible):
        spec.insert((k + 1) * len(order) // 3 + k, (int(n), 1.0))
    test = [_problem(g, n, table, bad) for n, bad in spec]
    filler = [_node(N_CAT, 0, synth.REQUEST_FLOATS), _node(N_CAT, 1, (1.0, 0.9, 1.0, 1.0, 0.9, 1.0))]
    nodefeatures = [filler] * (3 * len(test)) + test
    return {"nodefeatures": nodefeatures, "edge_indices": [_chain(len(p)) for p in nodefeatures],
            "labels": [[0] * N_SERVICES for _ in nodefeatures],
            "serviceFeature": {str(c + 1): table.qos[table.cat_ptr[c]:table.cat_ptr[c + 1]].tolist() for c in range(N_CAT)},
            "minCostList": [1.0 + 0.01 * b for b in range(len(nodefeatures))]}


def n_train(ds):
    return len(ds["nodefeatures"]) // 4 * 3


def problems_of(ds):
    return ds["nodefeatures"][n_train(ds):]


def task_counts(ds):
    return [len(nodes) - 1 for nodes in problems_of(ds)]


def slot_lists(ds, reduct, ssets=None, only=None):
    """addS's list of every task node of the test problems, empty ones included (loadDataOther without the drop); ``ssets``: a pick
    set per problem; ``only``: that test problem alone (a list of one)."""
    from gnnpn_sc_amd.loadData import addS
    sf = ds["serviceFeature"]
    div, mod = [], []
    for key in sf:
        div += [int(key) - 1] * len(sf[key])
        mod += list(range(len(sf[key])))
    out = []
    for b, nodes in enumerate(problems_of(ds)):
        if only is not None and b != only:
            continue
        cons = {c: [0] * 8 for c in range(1, len(sf) + 1)}
        for node in nodes:
            pair = node[-5:-3] + node[-2:]
            if node[0] == 1:
                for c in cons:
                    cons[c][-4:] = pair
            else:
                cons[node[:-6].index(1)][-8:-4] = pair
        index = [n[:-6].index(1) - 1 for n in nodes][1:]
        out.append(addS(range(len(div)), sf, cons, index, div, mod, reduct, ssets[b] if ssets else None))
    return out


def foreign_row(g):
    return [float(v) for v in np.r_[g.random(2), 0.9 + 0.1 * g.random(2)]]


def make_picks(ds, reduct, a_T, seed, foreign=0.1, mismatch=True):
    """Action rows [nTest, a_T, 8] float64: per problem one row per non-empty list IN NODE ORDER (the pairing is by position), then
    dummy rows (0, 1, 1, 1).  A row is a member of its slot's list at ``reduct`` (for reduct != 0 of the front without picks, any
    position of it, or of the front that the pick itself extends) or, about one in ten, a foreign row.  Among the problems with more than 64 lists the second has no rows, and
    (``mismatch``) the third one row too many and the fifth one too few; among the others every fifth has no rows.  Where a
    problem's rows exceed a_T the first such problem keeps a_T of them (too few), the others none."""
    g = np.random.default_rng(seed)
    lists_all = slot_lists(ds, reduct)
    inside_all = slot_lists(ds, 0) if reduct else lists_all
    acts = np.zeros((len(lists_all), a_T, 8))
    acts[:, :, 1:4] = 1.0
    big = small = cut = 0
    for b, lists in enumerate(lists_all):
        # reduct != 0: three rows in ten come from all the services inside the slot's bounds, not from the front alone — a pick
        # that the front keeps only because it is a pick (appended, or skipped when a newcomer would replace it)
        lists = [ins if reduct and g.random() < 0.3 else lst for lst, ins in zip(lists, inside_all[b]) if lst]
        rows = [foreign_row(g) if g.random() < foreign else list(lst[int(g.integers(0, len(lst)))]) for lst in lists]
        if len(lists) > 64:
            big += 1
            if big == 2:
                rows = []
            elif mismatch and big == 3:
                rows.append(foreign_row(g))
            elif mismatch and big == 5:
                rows.pop()
        else:
            small += 1
            if small % 5 == 4:
                rows = []
        if len(rows) > a_T:
            cut += 1
            rows = rows[:a_T] if cut == 1 else []
        if rows:
            acts[b, :len(rows), :4] = rows
    return acts


def layout(host):
    """What the host's tables (test_gpu_refine._host_tables' first result) say of the flat device tables: the status word per problem,
    prob_ptr and cand_ptr as exclusive scans of the list and candidate counts (a problem that raised counts 0), the largest list
    count and candidate count of a problem that did not raise."""
    status, prob_ptr, cand_ptr, max_slots, max_cand = [], [0], [0], 0, 0
    for h in host:
        if isinstance(h, Exception):
            status.append(STATUS_NO_SLOTS if "no categories" in str(h) else STATUS_ROWS_MISMATCH if "solution has" in str(h) else None)
            prob_ptr.append(prob_ptr[-1])
            continue
        status.append(STATUS_OK)
        cats = h[0]
        prob_ptr.append(prob_ptr[-1] + len(cats))
        for cat in cats:
            cand_ptr.append(cand_ptr[-1] + len(cat))
        max_slots = max(max_slots, len(cats))
        max_cand = max(max_cand, sum(len(cat) for cat in cats))
    return {"status": status, "prob_ptr": prob_ptr, "cand_ptr": cand_ptr, "max_slots": max_slots, "max_cand": max_cand}


def pick_sets(acts):
    """The pick set of every problem as WOA.start forms it: the rounded rows, dummy rows dropped."""
    out = []
    for rows in np.asarray(acts, dtype=np.float64)[:, :, :4].tolist():
        out.append({tuple(round(v, 5) for v in r) for r in rows if sum(r) != 3})
    return out


def rounded(row):
    return [round(float(v), 5) for v in row[:4]]


def protected_pick(ds, b, reduct, acts, col, val):
    """(acts', row index j, the rounded row) with a pick planted in test problem ``b`` that addS skips by: row j of ``acts[b]``
    becomes a service inside its slot's bounds that the front without picks does not keep, so that the slot's list with the pick
    set as it is (the pick is appended, or kept from being replaced) differs from the list with the row patched in ``col`` to
    ``val`` in the set's place — what patching the pick set by mistake would give.  None: no such row."""
    inside = [lst for lst in slot_lists(ds, 0, only=b)[0] if lst]
    front = [lst for lst in slot_lists(ds, reduct, only=b)[0] if lst]
    if len(inside) != len(front) or not np.any(acts[b, :len(front), :4].sum(1) != 3):
        return None
    for j, (all_in, kept) in enumerate(zip(inside, front)):
        for row in all_in:
            if row in kept:
                continue
            out = np.array(acts, dtype=np.float64)
            out[b, j, :4] = row
            key = rounded(row)
            moved = list(key)
            moved[col] = val
            ssets = pick_sets(out)
            trial = list(ssets)
            trial[b] = (ssets[b] - {tuple(key)}) | {tuple(moved)}
            if slot_lists(ds, reduct, ssets, only=b)[0] != slot_lists(ds, reduct, trial, only=b)[0]:
                return out, j, key
    return None


def host_tables(root, acts, reduct, patches=()):
    """test_gpu_refine._host_tables over the data set written under ``root`` (the host path reads ./data/QWS)."""
    import os
    from test_gpu_refine import _host_tables
    cwd = os.getcwd()
    os.chdir(root)
    try:
        return _host_tables("QWS", np.asarray(acts, dtype=np.float64), reduct, patches)
    finally:
        os.chdir(cwd)


def host_problems(root, acts, reduct):
    """The (services, constraints, solution | None) problems WOA.start hands to fine_tune for these action rows."""
    import os
    from gnnpn_sc_amd.loadData import loadDataOther
    rows = [[r for r in rows if sum(r) != 3] for rows in np.asarray(acts, dtype=np.float64)[:, :, :4].tolist()]
    cwd = os.getcwd()
    os.chdir(root)
    try:
        feats, cons, _mins = loadDataOther("QWS", reduct, sSetList=pick_sets(acts))
    finally:
        os.chdir(cwd)
    return [(feats[b], cons[b], rows[b] or None) for b in range(len(rows))]

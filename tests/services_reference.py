"""Helper of the service-id tests (not a test file): the host path of the candidate tables restated over indices, in plain
Python — ``addS`` run on (index, row) pairs so that the kept lists hold rows of the service table, ``WOA._prepare``'s pairing and
appended row, the mapping from a search's positions to services, and the scorer (``oracle.woa.objective`` over the rows the ids
name).  What gnnpn_woa_candidates_services, gnnpn_search_services and gnnpn_services_merit_f64 are compared with, ``==``
throughout.  The problems are tests/candidate_tables_reference.py's; tests/test_services_host.py holds this file against the
host path itself (the rows its indices name are ``slot_lists``' rows)."""
import numpy as np

import candidate_tables_reference as ctr
import descent_reference as ref

N_SLOTS = 50                                           # addS sizes its per-category lists for 50 categories


def service_rows(ds):
    """(rows [S][4], cat_ptr [T+1]) of the service table in the order addS walks it (category by category, table order): row s is
    what tables_from_dataset puts at ``qos[s]`` (test_services_host.py checks it)."""
    rows, cat_ptr = [], [0]
    for key in ds["serviceFeature"]:
        rows += [tuple(float(v) for v in r[-4:]) for r in ds["serviceFeature"][key]]
        cat_ptr.append(len(rows))
    return rows, cat_ptr


def adds_ids(rows, cat_ptr, constraints, service_index, reduct=0, sset=None):
    """loadData.addS with every entry carried as (row, index): the kept lists, as indices into ``rows``."""
    kept = [[] for _ in range(N_SLOTS)]
    front = [[(1.0, 0.0, 1.0, 1.0)] for _ in range(N_SLOTS)]
    for cat in range(len(cat_ptr) - 1):
        bounds = constraints[cat + 1]
        for s in range(cat_ptr[cat], cat_ptr[cat + 1]):
            entry = rows[s]
            q0, q1, cost, quality = entry
            if not (bounds[0] <= cost <= bounds[1] and bounds[2] <= quality <= bounds[3]):
                continue
            if not reduct:
                kept[cat].append(s)
                continue
            members, replaced = front[cat], False
            for x in range(len(members)):
                m = members[x]
                if sset and tuple(round(v, 5) for v in m) in sset:
                    continue
                if q0 < m[0] and q1 > m[1] and m[1] < reduct:
                    members[x] = entry
                    if not kept[cat]:
                        kept[cat].append(s)
                    else:
                        kept[cat][x] = s
                    replaced = True
                    break
                if (q0 > m[0] and q1 < m[1]) or q1 > reduct > q0:
                    break
            if not replaced and ((sset and tuple(round(v, 5) for v in entry) in sset) or q1 > reduct > q0):
                members.append(entry)
                kept[cat].append(s)
    return [list(kept[c]) for c in service_index]


def slot_ids(ds, reduct, ssets=None):
    """ctr.slot_lists over indices: per test problem, per task node (node order, empty lists included) the kept services."""
    rows, cat_ptr = service_rows(ds)
    n_cat = len(cat_ptr) - 1
    out = []
    for b, nodes in enumerate(ctr.problems_of(ds)):
        cons = {c: [0] * 8 for c in range(1, n_cat + 1)}
        for node in nodes:
            pair = node[-5:-3] + node[-2:]
            if node[0] == 1:
                for c in cons:
                    cons[c][-4:] = pair
            else:
                cons[node[:-6].index(1)][-8:-4] = pair
        index = [n[:-6].index(1) - 1 for n in nodes][1:]
        try:
            out.append((index, adds_ids(rows, cat_ptr, cons, index, reduct, ssets[b] if ssets else None)))
        except IndexError as e:                          # addS replaces past the end of a kept list
            out.append((index, e))
    return out


def named_tables(ds, acts, reduct=0, patches=(), action_ids=None):
    """Per test problem what woa_candidates_named adds to its tables, or None where the host path raises (a status word on the
    device, no room in the tables): dict(slot_node, slot_cat — one entry per non-empty list, node order —, cand_service — per list
    the kept services and, where WOA._prepare appends the paired row, the id ``action_ids`` [nTest, a_T] gives that action row or
    -1 —, start, seeded).  ``acts`` [nTest, a_T, 8]: the rows as the builder sees them (float32 rows widened)."""
    acts = np.asarray(acts, dtype=np.float64)
    rows, _cat_ptr = service_rows(ds)
    ssets = ctr.pick_sets(acts) if reduct else None
    out = []
    for b, (index, kept) in enumerate(slot_ids(ds, reduct, ssets)):
        if isinstance(kept, Exception):
            out.append(None)
            continue
        real = [k for k, r in enumerate(acts[b, :, :4].tolist()) if sum(r) != 3]
        lists = [(s + 1, index[s], ids) for s, ids in enumerate(kept) if ids]
        if (real and len(real) != len(lists)) or not lists:
            out.append(None)
            continue
        sol = [[round(float(v), 5) for v in acts[b, k, :4]] for k in real]
        for want, col, val in patches:
            for r in sol:
                if r == list(want):
                    r[col] = val
        tab = {"slot_node": [n for n, _c, _i in lists], "slot_cat": [c for _n, c, _i in lists], "cand_service": [], "start": [],
               "seeded": bool(real)}
        for j, (_n, _c, ids) in enumerate(lists):
            ids = list(ids)
            if real:
                members = [tuple(round(v, 5) for v in rows[s]) for s in ids]
                key = tuple(sol[j])
                if key not in members:
                    members.append(key)
                    ids.append(-1 if action_ids is None else int(action_ids[b][real[j]]))
                tab["start"].append(members.index(key))
            tab["cand_service"].append(ids)
        out.append(tab)
    return out


def flat(tabs):
    """(slot_node, slot_cat, cand_service) of the whole batch, as the device lays them out (a failed problem takes no room)."""
    node, cat, cand = [], [], []
    for t in tabs:
        if t is not None:
            node += t["slot_node"]
            cat += t["slot_cat"]
            for ids in t["cand_service"]:
                cand += ids
    return node, cat, cand


def map_services(tab, fitness, pos, n_nodes, ld):
    """(best_services [ld], node_services [n_nodes]) of one problem: ``tab`` its named_tables entry (None: failed), ``fitness``
    its best_fitness, ``pos`` its best_pos row.  Python list positions; a position outside its list names -1; a NaN merit, or no
    tables, -1 throughout."""
    best, nodes = [-1] * ld, [-1] * n_nodes
    if tab is None or fitness != fitness or len(tab["slot_node"]) > ld:
        return best, nodes
    for l, ids in enumerate(tab["cand_service"]):
        p = pos[l] + len(ids) if pos[l] < 0 else pos[l]
        if 0 <= p < len(ids):
            best[l] = nodes[tab["slot_node"][l]] = ids[p]
    return best, nodes


def score(qos_rows, ids, bounds, rounded=True):
    """(merit, n_rows) of the composition ``ids`` (one entry per node of a problem, -1: none) as gnnpn_services_merit_f64 defines
    it: oracle.woa.objective over the rows, rounded to 5 decimals where ``rounded``.  An id outside [-1, S): (NaN, -1); no rows:
    (NaN, 0)."""
    if any(i < -1 or i >= len(qos_rows) for i in ids):
        return float("nan"), -1
    rows = [tuple(round(float(v), 5) if rounded else float(v) for v in qos_rows[i]) for i in ids if i >= 0]
    if not rows:
        return float("nan"), 0
    return ref.merit(rows, bounds), len(rows)


# ---- the batch the mapping, the promise and the certificate run on (conditions: tests/test_services_host.py) --------------------------

NAMED_SEED, NAMED_PICK_SEED, NAMED_FAILED = ctr.SEARCH_SEED, 31, (70,)
TWIN_SHIFT = 1e-9                                      # far below half a unit of the fifth decimal


def named_dataset():
    """ctr's search batch (3 .. 200 task nodes) with one all-infeasible problem in its middle — a failed problem between good ones —
    and a planted twin: the service that most lists of the batch keep (the last of a category aside) gives the next service of its
    category its row, moved by 1e-9 in q0 — two services of equal rounded rows that the same lists keep.  Returns (ds, category,
    (first id, twin id))."""
    import copy
    from collections import Counter
    ds = copy.deepcopy(ctr.make_dataset(NAMED_SEED, ctr.SEARCH_COUNTS, NAMED_FAILED))
    _rows, cat_ptr = service_rows(ds)
    kept = Counter(s for _index, lists in slot_ids(ds, 0) for k in lists for s in k if s + 1 not in cat_ptr)
    first = kept.most_common(1)[0][0]
    cat = max(c for c in range(len(cat_ptr) - 1) if cat_ptr[c] <= first)
    sf = ds["serviceFeature"][str(cat + 1)]
    m = first - cat_ptr[cat]
    sf[m + 1] = list(sf[m])
    sf[m + 1][-4] = sf[m][-4] + TWIN_SHIFT
    return ds, cat, (first, first + 1)


def named_picks(ds, a_T=200, seed=NAMED_PICK_SEED, foreign=0.15, twin=None):
    """(acts [nTest, a_T, 8] f64, action_ids [nTest, a_T] i32) at reduct 0: per problem one row per non-empty list in node order —
    a member of the list or, about one in seven, a foreign row: a service of the table that the list does not keep — then dummy
    rows (0, 1, 1, 1) with id -1.  Every row is a row of the table, bit for bit, and action_ids names it: what ML2PNPipeline.run
    hands over.  ``twin`` (first id, twin id): wherever a list keeps both, the pick is the twin."""
    g = np.random.default_rng(seed)
    rows, _cat_ptr = service_rows(ds)
    kept_all = slot_ids(ds, 0)
    acts = np.zeros((len(kept_all), a_T, 8))
    acts[:, :, 1:4] = 1.0
    ids = np.full((len(kept_all), a_T), -1, dtype=np.int32)
    for b, (_index, kept) in enumerate(kept_all):
        lists = [k for k in kept if k]
        assert len(lists) <= a_T
        for j, k in enumerate(lists):
            if twin and twin[0] in k and twin[1] in k:
                s = twin[1]
            elif g.random() < foreign:
                s = int(g.integers(0, len(rows)))
                while s in k:
                    s = int(g.integers(0, len(rows)))
            else:
                s = k[int(g.integers(0, len(k)))]
            acts[b, j, :4] = rows[s]
            ids[b, j] = s
    return acts, ids

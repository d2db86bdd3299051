"""Helper of the pair-swap descent tests (not a test file): the search of gnnpn_descend_pairs_ragged_f64, of its windowed and of its
shortlist entry in plain Python, stated once and built on descent_reference.descend and merit — the contract the kernels are compared
with, field for field and bit for bit."""
import math

from descent_reference import descend, merit


def _settled(r):
    """Did the one-swap phase ``r`` end with a sweep that moved nothing?  (A move strictly lowers the merit.)"""
    s = r["sweeps"]
    return s >= 1 and r["history"][s - 1] == (r["history"][s - 2] if s >= 2 else r["start_fitness"])


def shortlists(cats, bounds, cur, m):
    """Per slot s the min(m, len) candidates c with the lowest merit of ``cur`` with slot s alone replaced by c — ordered by (merit,
    position) under plain <, a NaN after every number and NaNs by position, -0.0 equal to 0.0 — as ascending positions."""
    rows = [cats[s][cur[s]] for s in range(len(cats))]
    out = []
    for s, cat in enumerate(cats):
        keyed = []
        for c, row in enumerate(cat):
            rows[s] = row
            f = merit(rows, bounds)
            keyed.append((f != f, 0.0 if f != f else f, c))
        rows[s] = cat[cur[s]]
        out.append(sorted(c for _n, _f, c in sorted(keyed)[:m]))
    return out


def descend_pairs(cats, bounds, start, max_sweeps=16, max_rounds=4, max_span=0, max_rank=0, with_shortlist=False):
    """The one statement of the search, for the three entries.  One-swap descent (phase 0: exactly descent_reference.descend), then up
    to ``max_rounds`` rounds of: one pair sweep — for every slot pair i < j in lexicographic order (max_span > 0: only j < min(T, i +
    max_span + 1)), the composition with slots i and j replaced by (cats[i][a], cats[j][b]) for EVERY (a, b), current members
    included; the smallest merit under plain <, the lowest (a, b) among equals; a NaN never wins; the move is taken if it is strictly
    below the current merit — and, if the sweep moved, a one-swap descent from there.  A round whose pair sweep moved nothing is the
    last (it is counted).  max_rank = m > 0: the pair sweep forms ``shortlists`` of the composition it starts from and tries only
    (a, b) of S_i x S_j, in the order of k = ia * |S_j| + ib, the lowest k among equals; the shortlists stay as formed through the
    sweep.  converged says: no single swap and no pair within the span (and the shortlists) helps.  Returns dict(best_fitness,
    start_fitness, best_pos, best_rows, sweeps, moves, rounds, pair_moves, round_history, converged) and, ``with_shortlist`` (the
    shortlist entry's dict), shortlist: the last sweep's shortlists (None: no pair sweep ran, or m = 0)."""
    T = len(cats)
    r = descend(cats, bounds, start, max_sweeps)
    cur, fit, start_fitness = list(r["best_pos"]), r["best_fitness"], r["start_fitness"]
    sweeps, moves, settled = r["sweeps"], r["moves"], _settled(r)
    rounds, pair_moves, round_history, moved, lists = 0, 0, [], True, None
    for _ in range(max_rounds):
        moved = False
        rows = [cats[s][cur[s]] for s in range(T)]
        lists = shortlists(cats, bounds, cur, max_rank) if max_rank > 0 else None
        short = lists if lists is not None else [range(len(cat)) for cat in cats]
        for i in range(T):
            for j in range(i + 1, min(T, i + max_span + 1) if max_span > 0 else T):
                best_f, best_ab = math.inf, None
                for a in short[i]:
                    rows[i] = cats[i][a]
                    for b in short[j]:
                        rows[j] = cats[j][b]
                        f = merit(rows, bounds)
                        if f < best_f:
                            best_f, best_ab = f, (a, b)
                if best_ab is not None and best_f < fit:         # strictly
                    cur[i], cur[j] = best_ab
                    fit = best_f
                    pair_moves += 1
                    moved = True
                rows[i], rows[j] = cats[i][cur[i]], cats[j][cur[j]]
        rounds += 1
        if moved:
            r = descend(cats, bounds, cur, max_sweeps)
            cur, fit = list(r["best_pos"]), r["best_fitness"]
            sweeps += r["sweeps"]
            moves += r["moves"]
            settled = _settled(r)
        round_history.append(fit)
        if not moved:
            break
    round_history += [fit] * (max(max_rounds, 1) - len(round_history))
    return {"best_fitness": fit, "start_fitness": start_fitness, "best_pos": cur,
            "best_rows": [tuple(cats[s][cur[s]]) for s in range(T)], "sweeps": sweeps, "moves": moves, "rounds": rounds,
            "pair_moves": pair_moves, "round_history": round_history, "converged": int(rounds > 0 and not moved and settled),
            **({"shortlist": lists} if with_shortlist else {})}


def wall_problem(twice=False):
    """(cats, bounds, start) of two slots whose start is a one-swap optimum behind a wall: column 2's product must lie in [0.2, 0.3],
    the start rows give 0.81, either single swap 0.45 (still one violation, and a worse objective), both swaps 0.25.  ``twice``: the
    repairing rows stand twice in their lists, so four pairs tie."""
    a, b = (0.5, 0.5, 0.9, 1.0), (0.6, 0.5, 0.5, 1.0)
    cats = [[a, b, b], [a, b, b]] if twice else [[a, b], [a, b]]
    return cats, [0.2, 0.3, 0.0, 1.0], [0, 0]


def improving_pairs(cats, bounds, pos, fit):
    """Every (i, j, a, b), i < j, whose exchange of two slots in ``pos`` gives a merit strictly below ``fit`` (exhaustive)."""
    T = len(cats)
    rows = [cats[s][pos[s]] for s in range(T)]
    found = []
    for i in range(T):
        for j in range(i + 1, T):
            for a, ra in enumerate(cats[i]):
                rows[i] = ra
                for b, rb in enumerate(cats[j]):
                    rows[j] = rb
                    if merit(rows, bounds) < fit:
                        found.append((i, j, a, b))
            rows[i], rows[j] = cats[i][pos[i]], cats[j][pos[j]]
    return found

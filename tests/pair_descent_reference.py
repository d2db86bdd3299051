"""Helper of the pair-swap descent tests (not a test file): the search of gnnpn_descend_pairs_ragged_f64 in plain Python, built on
descent_reference.descend and merit — the contract the kernel is compared with, field for field and bit for bit."""
import math

from descent_reference import descend, merit


def _settled(r):
    """Did the one-swap phase ``r`` end with a sweep that moved nothing?  (A move strictly lowers the merit.)"""
    s = r["sweeps"]
    return s >= 1 and r["history"][s - 1] == (r["history"][s - 2] if s >= 2 else r["start_fitness"])


def descend_pairs(cats, bounds, start, max_sweeps=16, max_rounds=4):
    """One-swap descent (phase 0: exactly descent_reference.descend), then up to ``max_rounds`` rounds of: one pair sweep — for
    every slot pair i < j in lexicographic order, the composition with slots i and j replaced by (cats[i][a], cats[j][b]) for EVERY
    (a, b), current members included; the smallest merit under plain <, the lowest (a, b) among equals; a NaN never wins; the move is
    taken if it is strictly below the current merit — and, if the sweep moved, a one-swap descent from there.  A round whose pair
    sweep moved nothing is the last (it is counted).  Returns dict(best_fitness, start_fitness, best_pos, best_rows, sweeps, moves,
    rounds, pair_moves, round_history, converged)."""
    T = len(cats)
    r = descend(cats, bounds, start, max_sweeps)
    cur, fit, start_fitness = list(r["best_pos"]), r["best_fitness"], r["start_fitness"]
    sweeps, moves, settled = r["sweeps"], r["moves"], _settled(r)
    rounds, pair_moves, round_history, moved = 0, 0, [], True
    for _ in range(max_rounds):
        moved = False
        rows = [cats[s][cur[s]] for s in range(T)]
        for i in range(T):
            for j in range(i + 1, T):
                best_f, best_ab = math.inf, None
                for a, ra in enumerate(cats[i]):
                    rows[i] = ra
                    for b, rb in enumerate(cats[j]):
                        rows[j] = rb
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
            "pair_moves": pair_moves, "round_history": round_history, "converged": int(rounds > 0 and not moved and settled)}


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

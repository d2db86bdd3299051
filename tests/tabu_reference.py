"""Helper of the tabu-walk tests (not a test file): the search of gnnpn_descend_tabu_ragged_f64 in plain Python over
descent_reference.descend and merit — the contract the kernels are compared with, field for field and bit for bit — and the cases
the host and the GPU tests share (reference runs cached per session)."""
import functools
import math

import numpy as np

from descent_reference import descend, merit
import pair_descent_reference as pref
import pair_shortlist_reference as sref
from pair_window_reference import planted

FIELDS = ("best_fitness", "start_fitness", "sweeps", "moves", "steps", "best_step", "stalled")


def descend_tabu(cats, bounds, start, max_sweeps=16, max_steps=32, tenure=None, with_trace=False):
    """The one statement of the walk.  Phase 0: descent_reference.descend (up to ``max_sweeps``); best = cur, no move is tabu.  Step
    t = 1 .. max_steps: for every slot j in order and every position c != cur[j], f = the merit of cur with slot j replaced by c;
    (j, c) is tabu iff expire[j][c] >= t and admissible iff it is not tabu or f < best_f (strict); the admissible move with the
    smallest f under plain < is taken, the lowest (j, c) among equals, a NaN never — whether or not f is below the current merit —
    and the position left gets expire = t + tenure.  No admissible move: stalled, the walk ends, the step is not counted.  best
    follows under strict <.  Polish: where steps > 0, best_step == steps and the walk did not stall, descend runs once more from
    best (its sweeps and moves are added, its result is the result).  Returns dict(best_fitness, start_fitness, best_pos, best_rows,
    sweeps, moves, history [max(max_steps, 1)]: the best merit after every step, past the last step the last such value (before the
    polish; max_steps = 0: phase 0's merit), walk [steps]: the current merit after every step taken (the kernels fill NaN behind
    it), steps, best_step, stalled) and, ``with_trace``, trace: per step (t, slot, position, position left, was tabu, merit, best
    merit before the step) and polished: (ran, moves)."""
    if tenure is None:
        from gnnpn_sc_amd.ops import DEFAULT_TENURE as tenure
    T = len(cats)
    r = descend(cats, bounds, start, max_sweeps)
    cur, fit = list(r["best_pos"]), r["best_fitness"]
    best, best_f, best_step = list(cur), fit, 0
    sweeps, moves = r["sweeps"], r["moves"]
    expire = [[0] * len(cat) for cat in cats]
    rows = [cats[j][cur[j]] for j in range(T)]
    history, walk, trace, steps, stalled = [], [], [], 0, 0
    for t in range(1, max_steps + 1):
        pick_f, pick = math.inf, None
        for j in range(T):
            for c, row in enumerate(cats[j]):
                if c == cur[j]:
                    continue
                rows[j] = row
                f = merit(rows, bounds)
                tabu = expire[j][c] >= t
                if (not tabu or f < best_f) and f < pick_f:      # the lowest (j, c) among equals; a NaN never wins
                    pick_f, pick = f, (j, c, tabu)
            rows[j] = cats[j][cur[j]]
        if pick is None:
            stalled = 1
            break
        j, c, was_tabu = pick
        trace.append((t, j, c, cur[j], was_tabu, pick_f, best_f))
        expire[j][cur[j]] = t + tenure
        cur[j], rows[j], fit, steps = c, cats[j][c], pick_f, t
        walk.append(fit)
        if fit < best_f:
            best, best_f, best_step = list(cur), fit, t
        history.append(best_f)
    history += [best_f] * (max(max_steps, 1) - len(history))
    polished = (False, 0)
    if steps > 0 and best_step == steps and not stalled:
        p = descend(cats, bounds, best, max_sweeps)
        best, best_f = list(p["best_pos"]), p["best_fitness"]
        sweeps += p["sweeps"]
        moves += p["moves"]
        polished = (True, p["moves"])
    out = {"best_fitness": best_f, "start_fitness": r["start_fitness"], "best_pos": best,
           "best_rows": [tuple(cats[j][best[j]]) for j in range(T)], "sweeps": sweeps, "moves": moves, "history": history, "walk": walk,
           "steps": steps, "best_step": best_step, "stalled": stalled}
    if with_trace:
        out.update(trace=trace, polished=polished)
    return out


def returns_within_tenure(run, tenure):
    """The steps of ``run`` (with_trace) that take a slot back to a position it left within the last ``tenure`` steps although
    their merit is not below the best before them: none, by the contract."""
    left, bad = {}, []
    for t, j, c, was, _tabu, f, best_before in run["trace"]:
        if (j, c) in left and t - left[j, c] <= tenure and not f < best_before:
            bad.append(t)
        left[j, was] = t
    return bad


def single_rows(T=3):
    """(cats, bounds, start): every list has one row — no move exists."""
    g = np.random.default_rng(11)
    return [[(float(g.random()), 0.95, 1.0, 1.0)] for _ in range(T)], [0.0, 1.0, 0.0, 1.0], [0] * T


def one_slot():
    """T = 1, five rows, started off its best."""
    return [[(0.3, 0.5, 0.9, 0.9), (0.2, 0.6, 0.9, 0.9), (0.25, 0.6, 0.9, 0.9), (0.1, 0.4, 0.9, 0.9), (0.15, 0.5, 0.9, 0.9)]], [0.0, 1.0, 0.0, 1.0], [0]


def wall_wide(T=131, i=63, j=64):
    """planted(T, nfill=1) — every filler list has one row, so the wall's two slots hold the only moves — with the column-2 wall
    across two leaf blocks of np.sum: the one-swap optimum (poor, poor) is left by the worse single swap at step 1 and repaired at
    step 2, so best_step = 2 > 0 in the workgroup form's recursion above 128 slots."""
    return planted(13100 + T, T, wall2=(i, j), nfill=1)


def outside_start():
    """The wall problem with a start outside its second list: not searched."""
    cats, bounds, _start = pref.wall_problem()
    return cats, bounds, [0, 2]


# name -> (tables, dict(max_steps=, tenure=, ...), wide)
SEED_RUNS = ((0, 3), (2, 3), (3, 3), (32, 0), (32, 3), (32, 5))


def _cases():
    c = {}
    seeds = sref._seeds_tables()
    for wide in (None, True):
        w = "_wide" if wide else ""
        for steps, tenure in SEED_RUNS:
            c[f"seeds_s{steps}_t{tenure}{w}"] = (seeds, dict(max_steps=steps, tenure=tenure), wide)
        c[f"seeds_s32_t3_sweeps0{w}"] = (seeds, dict(max_steps=32, tenure=3, max_sweeps=0), wide)
        c[f"small{w}"] = ((sref.duplicated_rows(), sref.nan_row_problem(), one_slot(), single_rows(), pref.wall_problem()),
                          dict(max_steps=6, tenure=2), wide)
    c["t64"] = (sref._t64_tables(), dict(max_steps=32, tenure=3), None)
    c["long"] = (sref._long_tables(), dict(max_steps=32, tenure=3), None)
    c["long_wide"] = ((sref.long_list_wide(),), dict(max_steps=16, tenure=3), True)
    c["planted65"] = ((planted(6501, 65, wall2=(3, 40), mins=(10, 64), nfill=6),), dict(max_steps=12, tenure=4), True)
    c["planted129"] = ((planted(12901, 129, wall2=(63, 64), wall3=(0, 128), mins=(70, 100), nfill=6),), dict(max_steps=12, tenure=4), True)
    c["planted257"] = ((planted(25701, 257, wall2=(127, 128), wall3=(191, 192), mins=(200, 207), nfill=6),), dict(max_steps=12, tenure=4), True)
    c["wall131"] = ((wall_wide(),), dict(max_steps=4, tenure=2), True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def run(table_key, index, max_sweeps, max_steps, tenure):
    """One cached reference run (with its trace): table ``index`` of CASES[table_key]'s tables."""
    return descend_tabu(*CASES[table_key][0][index], max_sweeps=max_sweeps, max_steps=max_steps, tenure=tenure, with_trace=True)


@functools.lru_cache(maxsize=None)
def case_want(name):
    """The reference runs of a case.  The wide cases over the same tables share the lane case's runs."""
    tables, kw, _wide = CASES[name]
    key = name[:-5] if name.endswith("_wide") and name[:-5] in CASES and CASES[name[:-5]][0] is tables else name
    return tuple(run(key, p, kw.get("max_sweeps", 16), kw["max_steps"], kw["tenure"]) for p in range(len(tables)))


def seeds_runs(max_steps, tenure, max_sweeps=16):
    """The 20 SEEDS tables at one setting (cached; the GPU cases' settings share these runs)."""
    return tuple(run("seeds_s0_t3", p, max_sweeps, max_steps, tenure) for p in range(len(sref._seeds_tables())))

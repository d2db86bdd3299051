"""Helper of the pair-move tabu walk's tests (not a test file): the search of gnnpn_descend_tabu_pairs_ragged_f64 in plain Python over
descent_reference.descend and merit and pair_descent_reference.shortlists — the contract the kernels are compared with, field for
field and bit for bit — and the cases the host and the GPU tests share (reference runs cached per session)."""
import functools
import math

from descent_reference import descend, merit
from pair_descent_reference import shortlists, wall_problem
import pair_shortlist_reference as sref
from pair_window_reference import planted
import tabu_reference as tref

FIELDS = tref.FIELDS + ("pair_steps",)


def descend_tabu_pairs(cats, bounds, start, max_sweeps=16, max_steps=32, tenure=None, max_rank=None, max_span=0, with_trace=False):
    """The one statement of the walk.  Phase 0: descent_reference.descend (up to ``max_sweeps``); best = cur, no position is tabu.
    Step t = 1 .. max_steps.  Singles, the tabu walk's: every slot j in order and every position c != cur[j] of its whole list, f =
    the merit of cur with slot j replaced; tabu iff expire[j][c] >= t.  Then ``shortlists`` of cur (max_rank = 0, or at least a
    list's length: the whole list; formed anew every step; a shortlist may hold cur[j]) and the pairs: every i < j in lexicographic
    order (max_span = s > 0: only j <= i + s), every a of S_i and b of S_j, positions ascending, with a != cur[i] and b != cur[j],
    f = the merit with both slots replaced; tabu iff expire[i][a] >= t or expire[j][b] >= t.  A move is admissible iff it is not
    tabu or f < best_f (strict); the admissible move with the smallest f under plain < is taken — a NaN never, a single before a
    pair among equals, singles by the lowest (j, c), pairs by the lowest (i, j, a, b) — whether or not f is below the current merit,
    and every slot that moves bars the position it leaves: expire = t + tenure.  No admissible move: stalled, the walk ends, the
    step is not counted.  best follows under strict <; the end (polish, padding) is tabu_reference.descend_tabu's.  Returns that
    function's dict plus pair_steps (the steps that took a pair) and, ``with_trace``, trace: per step (t, ((slot, position,
    position left, was tabu), ... one or two ...), merit, best merit before the step) and polished: (ran, moves)."""
    if tenure is None:
        from gnnpn_sc_amd.ops import DEFAULT_TENURE as tenure
    if max_rank is None:
        from gnnpn_sc_amd.ops import DEFAULT_PAIR_RANK as max_rank
    T = len(cats)
    r = descend(cats, bounds, start, max_sweeps)
    cur, fit = list(r["best_pos"]), r["best_fitness"]
    best, best_f, best_step = list(cur), fit, 0
    sweeps, moves = r["sweeps"], r["moves"]
    expire = [[0] * len(cat) for cat in cats]
    rows = [cats[j][cur[j]] for j in range(T)]
    history, walk, trace, steps, stalled, pair_steps = [], [], [], 0, 0, 0
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
                    pick_f, pick = f, ((j, c, tabu),)
            rows[j] = cats[j][cur[j]]
        short = shortlists(cats, bounds, cur, max_rank if max_rank > 0 else max(len(cat) for cat in cats))
        for i in range(T):
            for j in range(i + 1, min(T, i + max_span + 1) if max_span > 0 else T):
                for a in short[i]:
                    if a == cur[i]:
                        continue
                    rows[i] = cats[i][a]
                    for b in short[j]:
                        if b == cur[j]:
                            continue
                        rows[j] = cats[j][b]
                        f = merit(rows, bounds)
                        tabu_a, tabu_b = expire[i][a] >= t, expire[j][b] >= t
                        if (not (tabu_a or tabu_b) or f < best_f) and f < pick_f:      # strict: a single wins over an equal pair
                            pick_f, pick = f, ((i, a, tabu_a), (j, b, tabu_b))
                rows[i], rows[j] = cats[i][cur[i]], cats[j][cur[j]]
        if pick is None:
            stalled = 1
            break
        trace.append((t, tuple((j, c, cur[j], was) for j, c, was in pick), pick_f, best_f))
        for j, c, _was in pick:
            expire[j][cur[j]] = t + tenure
            cur[j], rows[j] = c, cats[j][c]
        fit, steps = pick_f, t
        pair_steps += len(pick) == 2
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
           "steps": steps, "best_step": best_step, "stalled": stalled, "pair_steps": pair_steps}
    if with_trace:
        out.update(trace=trace, polished=polished)
    return out


def returns_within_tenure(run, tenure):
    """The steps of ``run`` (with_trace) that take a slot — either component of a pair — back to a position it left within the last
    ``tenure`` steps although their merit is not below the best before them: none, by the contract."""
    left, bad = {}, []
    for t, parts, f, best_before in run["trace"]:
        if any((j, c) in left and t - left[j, c] <= tenure for j, c, _was, _tabu in parts) and not f < best_before:
            bad.append(t)
        for j, _c, was, _tabu in parts:
            left[j, was] = t
    return bad


# name -> (tables, dict(max_steps=, tenure=, max_rank=, max_span=, ...), wide); (steps, tenure, rank, span) of the SEEDS runs
SEED_RUNS = ((0, 3, 2, 0), (2, 3, 2, 0), (32, 3, 1, 0), (32, 3, 2, 0), (32, 3, 4, 1), (32, 0, 0, 0))


def _kw(steps, tenure, rank, span, **more):
    return dict(max_steps=steps, tenure=tenure, max_rank=rank, max_span=span, **more)


def _cases():
    c = {}
    seeds = sref._seeds_tables()
    small = (sref.duplicated_rows(), sref.nan_row_problem(), tref.one_slot(), tref.single_rows(), wall_problem())
    for wide in (None, True):
        w = "_wide" if wide else ""
        for steps, tenure, rank, span in SEED_RUNS:
            c[f"seeds_s{steps}_t{tenure}_r{rank}_w{span}{w}"] = (seeds, _kw(steps, tenure, rank, span), wide)
        c[f"seeds_s32_t3_r2_w0_sweeps0{w}"] = (seeds, _kw(32, 3, 2, 0, max_sweeps=0), wide)
        c[f"small{w}"] = (small, _kw(6, 2, 2, 0), wide)
    c["t64"] = (sref._t64_tables(), _kw(8, 3, 2, 0), None)
    c["long"] = (sref._long_tables(), _kw(8, 3, 8, 0), None)
    c["long_wide"] = ((sref.long_list_wide(),), _kw(6, 3, 4, 2), True)
    c["planted65"] = ((planted(6501, 65, wall2=(3, 40), mins=(10, 64), nfill=6),), _kw(6, 4, 2, 0), True)
    c["planted129"] = ((planted(12901, 129, wall2=(63, 64), wall3=(0, 128), mins=(70, 100), nfill=6),), _kw(6, 4, 2, 2), True)
    c["planted257"] = ((planted(25701, 257, wall2=(127, 128), wall3=(191, 192), mins=(200, 207), nfill=6),), _kw(6, 4, 2, 1), True)
    c["wall131"] = ((tref.wall_wide(),), _kw(2, 2, 2, 1), True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def run(table_key, index, max_sweeps, max_steps, tenure, max_rank, max_span):
    """One cached reference run (with its trace): table ``index`` of CASES[table_key]'s tables."""
    return descend_tabu_pairs(*CASES[table_key][0][index], max_sweeps=max_sweeps, max_steps=max_steps, tenure=tenure, max_rank=max_rank,
                              max_span=max_span, with_trace=True)


@functools.lru_cache(maxsize=None)
def case_want(name):
    """The reference runs of a case.  The wide cases over the same tables share the lane case's runs."""
    tables, kw, _wide = CASES[name]
    key = name[:-5] if name.endswith("_wide") and name[:-5] in CASES and CASES[name[:-5]][0] is tables else name
    return tuple(run(key, p, kw.get("max_sweeps", 16), kw["max_steps"], kw["tenure"], kw["max_rank"], kw["max_span"])
                 for p in range(len(tables)))


def seeds_runs(max_steps, tenure, max_rank, max_span=0, max_sweeps=16):
    """The 20 SEEDS tables at one setting (cached; the GPU cases' settings share these runs)."""
    return tuple(run("seeds_s0_t3_r2_w0", p, max_sweeps, max_steps, tenure, max_rank, max_span) for p in range(len(sref._seeds_tables())))

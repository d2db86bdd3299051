"""Helper of the descent tests (not a test file): the one-swap coordinate descent of gnnpn_descend_ragged_f64 in plain Python over
``oracle.woa.objective`` — the contract the kernels are compared with, field for field and bit for bit — and the packing of
WOA._prepare-style tables into the flat operands of ops.descend_ragged."""
import math

from oracle import woa as owoa


def merit(rows, bounds):
    """violate + objFunc of one composition, as ES-WOA forms it (oracle/woa.py)."""
    v, o = owoa.objective(rows, [[[bounds[0], bounds[1]]], [[bounds[2], bounds[3]]]])
    return v + o


def descend(cats, bounds, start, max_sweeps=16):
    """cats: per slot the list of (q0, q1, q2, q3) tuples (an appended foreign row included); bounds: [lo2, hi2, lo3, hi3]; start: a
    position per slot, or None (position 0 of every list).  Returns dict(best_fitness, start_fitness, best_pos, best_rows, history,
    sweeps, moves)."""
    T = len(cats)
    cur = list(start) if start is not None else [0] * T
    rows = [cats[j][cur[j]] for j in range(T)]
    fit = start_fitness = merit(rows, bounds)
    history, sweeps, moves = [], 0, 0
    for _ in range(max_sweeps):
        improved = False
        for j in range(T):
            best_f, best_c = math.inf, -1
            for c, row in enumerate(cats[j]):
                rows[j] = row
                f = merit(rows, bounds)
                if f < best_f:                       # the lowest position among equals; a NaN never wins
                    best_f, best_c = f, c
            if best_c >= 0 and best_f < fit:         # strictly
                cur[j], fit = best_c, best_f
                moves += 1
                improved = True
            rows[j] = cats[j][cur[j]]
        sweeps += 1
        history.append(fit)
        if not improved:
            break
    history += [fit] * (max_sweeps - sweeps)
    return {"best_fitness": fit, "start_fitness": start_fitness, "best_pos": cur, "best_rows": [tuple(r) for r in rows],
            "history": history, "sweeps": sweeps, "moves": moves}


def improving_swaps(cats, bounds, pos, fit):
    """Every (slot, position) whose single swap into ``pos`` gives a merit strictly below ``fit`` (exhaustive)."""
    rows = [cats[j][pos[j]] for j in range(len(cats))]
    found = []
    for j, cat in enumerate(cats):
        for c, row in enumerate(cat):
            rows[j] = row
            if merit(rows, bounds) < fit:
                found.append((j, c))
        rows[j] = cat[pos[j]]
    return found


def prepare(problems):
    """[(cats, bounds, start | None)] of (services, constraints, solution | None) problems, as WOA._prepare makes the tables."""
    from gnnpn_sc_amd import WOA
    out = []
    for services, cons, sol in problems:
        cats, _len0, start, _rows, bounds = WOA._prepare(services, cons, sol)
        out.append((cats, bounds, start))
    return out


def pack(tables):
    """The flat operands of ops.descend_ragged for [(cats, bounds, start | None)]: prob_ptr, cand_ptr, cand rows, bounds, start_pos
    (-1 for every slot of a problem without a start), as lists."""
    prob_ptr, cand_ptr, flat, bounds, start_pos = [0], [0], [], [], []
    for cats, bd, start in tables:
        for cat in cats:
            flat.extend(cat)
            cand_ptr.append(cand_ptr[-1] + len(cat))
        prob_ptr.append(prob_ptr[-1] + len(cats))
        start_pos.extend(start if start is not None else [-1] * len(cats))
        bounds.append(list(bd))
    return prob_ptr, cand_ptr, flat, bounds, start_pos

"""ML+2PN scorer behind the reference's entry points (/root/reference/src/ML2PN.py): ``calc``
(:6-12) and ``check(dataset, serCategory, epoch)`` (:15-56) — same CWD-relative artefact files,
same printed line ``<epoch> <score>``.  Host code in the reference as well (json + float64 numpy
over a few thousand rows); ``infer`` is the new part: it PRODUCES the artefacts ``check`` reads by
running the device pipeline, which the reference does inside its training drivers
(trainML.py:146-149, trainPNHigh.py:131-144).
"""
import json
import os

import numpy as np

from .loadData import loadDataPN


def calc(qos, cons):
    """0.5*(mean q0 + 1 - min q1) + one penalty per global constraint whose product QoS is out of
    bounds (ML2PN.py:6-12); float64."""
    obj = 0.5 * (np.average(qos[0]) + 1 - np.min(qos[1]))
    for col, (lo, hi) in zip((2, 3), cons):
        prod = np.cumprod(qos[col])[-1]
        if prod < lo or prod > hi:
            obj += 1
    return obj


def score(features_k1, min_cost, all_actions, serCategory):
    """The arithmetic of check (ML2PN.py:20-55) on in-memory structures -> mean(minCost / calc)."""
    qosNum = 4
    n = len(features_k1)
    n_train, n_test = n // 4 * 3, n // 4
    total = 0.0
    for j in range(n_test):
        picked = [all_actions[i][j][:qosNum] for i in range(serCategory)]
        picked = [a for a in picked if sum(a) != 3]                    # dummy rows [0,1,1,1] (:41-43)
        row0 = features_k1[n_train + j][0]
        cons = [row0[qosNum + 1:][:2], row0[qosNum + 1:][2:]]          # :51
        qos = [[a[i] for a in picked] for i in range(qosNum)]
        total += min_cost[n_train + j] / calc(qos, cons)
    return total / n_test


def check(dataset, serCategory, epoch):
    features, _ = loadDataPN(epoch=-1, dataset=dataset, serviceNumber=1)          # :19
    with open(f"./data/{dataset}/minCostList.data", "r") as f:
        min_cost = json.load(f)
    url = f"./solutions/pretrained/{dataset}-PNHigh.txt" if epoch == -1 else \
        f"./solutions/PNHigh/{dataset}/allActions{epoch}.txt"                     # :25-28
    with open(url) as f:
        all_actions = json.load(f)
    result = score(features, min_cost, all_actions, serCategory)
    print(epoch, result)                                                          # :57
    return result


def infer(dataset, net, low, high, n_per, epoch=-1, device="cuda:0", batch_size=128, precision="f32", woa=None, samples=1,
          sample_seed=None, descend=None, all_starts=False, pair_rounds=None):
    """Run ML+2PN inference over ``./data/<dataset>`` on the GPU and write the two artefacts that
    ``check`` reads: the rankings of ALL problems (trainML.py:146-149 format, [P][S] ints) and the
    High-level actions of the test quarter (trainPNHigh.py:133-144 format, [T][nTest][8]).
    ``precision``: arithmetic of the recurrent products and of the large-graph GIN layers — "f32" by default here (the artefact
    files are the reference's hand-off format: the parity path), "split" = what bench.py measures (the exact
    three-piece products: same selections on every pinned problem).
    ``woa``: a dict (popSize, MAX_Iter, reduct, seed) — then the test quarter's actions are also refined on the device
    (ML2PNPipeline.refine) and ``./solutions/WOA/<dataset>/ML+2PN+WOA.txt`` written as the WOA approach writes it (problem
    ``idx`` on stream ``seed + idx``; seed None: fresh seeds).
    ``samples`` > 1: best-of-N decoding (ML2PNPipeline.best_of): per problem the greedy answer or one of samples-1 sampled
    High decodes, whichever has the smallest R; the refinement then starts from it.  ``sample_seed``: the draws' seed
    (batch i of the run uses replica streams of sample_seed + i); None: fresh OS entropy.
    ``descend``: a number of sweeps (>= 1) — then the test quarter's actions are improved by one-swap descent on the device
    (pipeline.descend, at ``woa``'s reduct or 0) and ``./solutions/WOA/<dataset>/ML+2PN+descent.txt`` written in the same format;
    together with ``woa`` the ES-WOA run starts from the descended composition.
    ``all_starts`` (with samples > 1 and descend): the test quarter's rows of EVERY replica are kept per batch and descent runs from
    all of them (pipeline.descend_starts), the lowest local optimum per problem kept: ``ML+2PN+multistart.txt`` in place of
    ``ML+2PN+descent.txt``; with ``woa`` ES-WOA starts from that winner.  The PNHigh artefact is the best-of winner by R either way.
    ``pair_rounds`` (>= 1, with descend): pair-swap descent with that many rounds allowed in place of the one-swap descent
    (pipeline.descend_pairs / descend_starts_pairs): ``ML+2PN+pairs.txt`` (``ML+2PN+multistart+pairs.txt`` with all_starts) in
    place of the descent artefact, its format plus the per-problem rounds, pair_moves and converged; ES-WOA starts from its result.
    ``infer_pairs_windowed`` is this run with the pair-swap descent over a window of slots."""
    stage = _stage_asked("infer", descend, pair_rounds)
    return _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, woa, samples, sample_seed, descend, all_starts, stage)


def infer_pairs_windowed(dataset, net, low, high, n_per, epoch=-1, device="cuda:0", batch_size=128, precision="f32", samples=1,
                         sample_seed=None, descend=16, pair_rounds=4, pair_span=0):
    """``infer`` with ``descend`` and ``pair_rounds`` whose pair-swap descent takes any number of slots and exchanges only slots at most
    ``pair_span`` apart (>= 0; 0: every pair; pipeline.descend_pairs_windowed): ``ML+2PN+pairs.txt`` in ``infer``'s format plus ``span``.
    A function of its own because ``infer``'s parameter list is pinned by the host tests; without ``woa`` and ``all_starts``, which
    stay with the full sweep of at most 64 slots."""
    stage = _stage("infer_pairs_windowed", "descend_pairs_windowed", descend, pair_rounds, pair_span)
    return _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, None, samples, sample_seed, descend, False, stage)


def infer_pairs_shortlist(dataset, net, low, high, n_per, epoch=-1, device="cuda:0", batch_size=128, precision="f32", samples=1,
                          sample_seed=None, descend=16, all_starts=False, pair_rounds=4, pair_span=0, pair_rank=0):
    """``infer_pairs_windowed`` whose pair sweeps look only at the ``pair_rank`` best candidates of each slot (>= 0; 0: all;
    pipeline.descend_pairs_shortlist): ``ML+2PN+pairs.txt`` in ``infer``'s format plus ``span`` and ``top``.  With ``all_starts`` (and
    samples > 1) the descent runs from every replica (pipeline.descend_starts_pairs_shortlist): ``ML+2PN+multistart+pairs.txt``.
    Without ``woa``, whose start takes the full pair sweep of at most 64 slots."""
    stage = _stage("infer_pairs_shortlist", "descend_pairs_shortlist", descend, pair_rounds, pair_span, pair_rank)
    return _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, None, samples, sample_seed, descend, all_starts, stage)


def infer_tabu(dataset, net, low, high, n_per, epoch=-1, device="cuda:0", batch_size=128, precision="f32", samples=1, sample_seed=None,
               descend=16, all_starts=False, tabu_steps=32, tenure=None):
    """``infer`` with ``descend`` whose one-swap optimum is left by a tabu walk of up to ``tabu_steps`` steps (>= 0; ``tenure`` >= 0,
    None: ops.DEFAULT_TENURE; pipeline.descend_tabu): ``ML+2PN+tabu.txt`` in ``infer``'s format plus the per-problem ``steps``,
    ``best_step`` and ``stalled``, and ``tabu_steps`` / ``tenure``.  With ``all_starts`` (and samples > 1) the walk runs from every
    replica (pipeline.descend_starts_tabu): ``ML+2PN+multistart+tabu.txt``.  Without ``woa`` and without pair sweeps.  A function of
    its own because ``infer``'s parameter list is pinned by the host tests."""
    from . import ops
    stage = _stage("infer_tabu", "descend_tabu", descend, tabu_steps, ops.DEFAULT_TENURE if tenure is None else tenure)
    return _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, None, samples, sample_seed, descend, all_starts, stage)


def infer_tabu_pairs(dataset, net, low, high, n_per, epoch=-1, device="cuda:0", batch_size=128, precision="f32", samples=1, sample_seed=None,
                     descend=16, all_starts=False, tabu_steps=32, tenure=None, pair_rank=None, pair_span=0):
    """``infer_tabu`` whose step may take a pair swap of the ``pair_rank`` best candidates of two slots at most ``pair_span`` apart
    (>= 0; a rank of None: ops.DEFAULT_PAIR_RANK, of 0: whole lists; a span of 0: every slot pair; pipeline.descend_tabu_pairs):
    ``ML+2PN+tabu+pairs.txt`` in ``infer_tabu``'s format plus the per-problem ``pair_steps`` and the settings ``top`` and ``span``.
    With ``all_starts`` (and samples > 1) from every replica (pipeline.descend_starts_tabu_pairs):
    ``ML+2PN+multistart+tabu+pairs.txt``.  Without ``woa``.  A function of its own, as ``infer_tabu`` is."""
    from . import ops
    stage = _stage("infer_tabu_pairs", "descend_tabu_pairs", descend, tabu_steps, ops.DEFAULT_TENURE if tenure is None else tenure,
                   ops.DEFAULT_PAIR_RANK if pair_rank is None else pair_rank, pair_span)
    return _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, None, samples, sample_seed, descend, all_starts, stage)


def infer_services(dataset, net, low, high, n_per, epoch=-1, device="cuda:0", batch_size=128, precision="f32", woa=None, samples=1,
                   sample_seed=None, descend=None, all_starts=False, pair_rounds=None, pair_span=None, pair_rank=None):
    """``infer`` (with ``pair_span`` / ``pair_rank``: ``infer_pairs_windowed`` / ``infer_pairs_shortlist``) whose last search stage
    also says which services its compositions consist of: every artefact of that run as before, plus
    ``./solutions/WOA/<dataset>/ML+2PN+services.txt`` — per test problem the list of [node, category, service] (the node's position
    in its workflow graph, its 0-based category, the row of the service table; -1: a row of the pointer network that is no kept
    service and has no id), the merit ``pipeline.score_services`` gives that composition, the stage's best_fitness and the row
    count.  Needs ``descend`` or ``woa``.  A function of its own because ``infer``'s parameter list is pinned by the host tests."""
    if descend is None and woa is None:
        raise ValueError("ML2PN.infer_services: needs descend or woa (the services of a searched composition)")
    stage = _stage_asked("infer_services", descend, pair_rounds, pair_span, pair_rank)
    return _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, woa, samples, sample_seed, descend, all_starts, stage,
                  services=True)


# What this module adds to a stage of pipeline.STAGES, by its method: the least value of each option; what a call without ``descend``, without
# an option or with one below its least value is told; the ``infer*`` function that runs it; its part of the artefact's file name; the
# per-problem flag the artefact lists beside the stage's row_keys; the keys under which it lists the options' values (None: not listed).
RUNS = {
    "descend": ((), "", "infer", "", None, ()),
    "descend_pairs": ((1,), "pair_rounds needs descend and at least one round", "infer", "pairs", "converged", (None,)),
    "descend_pairs_windowed": ((1, 0), "pair_span needs descend, at least one round and a span >= 0", "infer_pairs_windowed", "pairs",
                               "converged", (None, "span")),
    "descend_pairs_shortlist": ((1, 0, 0), "pair_rank needs descend, at least one round, a span >= 0 and a rank >= 0", "infer_pairs_shortlist",
                                "pairs", "converged", (None, "span", "top")),
    "descend_tabu": ((0, 0), "tabu_steps needs descend, a number of steps >= 0 and a tenure >= 0", "infer_tabu", "tabu", "stalled",
                     ("tabu_steps", "tenure"))}


# The stages of pipeline.MORE_STAGES, in RUNS' format: a table of its own beside RUNS, as MORE_STAGES is beside STAGES.
MORE_RUNS = {
    "descend_tabu_pairs": ((0, 0, 0, 0), "pair_moves needs descend, a number of steps >= 0, a tenure >= 0, a rank >= 0 and a span >= 0",
                           "infer_tabu_pairs", "tabu+pairs", "stalled", ("tabu_steps", "tenure", "top", "span"))}


def run_named(name):
    """The row of that stage: RUNS' first, then MORE_RUNS'."""
    return RUNS[name] if name in RUNS else MORE_RUNS[name]


def stage_given(pair_rounds=None, pair_span=None, pair_rank=None, tabu_steps=None, pair_moves=None):
    """The stage (its name in pipeline.STAGES or MORE_STAGES) that the options given — not None — ask for: the one that takes the last
    of them.  ``pair_moves``: the rank of the tabu walk's pair moves."""
    return ("descend_tabu_pairs" if pair_moves is not None else "descend_tabu" if tabu_steps is not None else "descend_pairs_shortlist" if pair_rank is not None else
            "descend_pairs_windowed" if pair_span is not None else "descend_pairs" if pair_rounds is not None else "descend")


def stage_ok(name, descend, *values):
    """The precondition of a stage with options: ``descend`` is given, and so is every option, none below its least value."""
    return not values or (descend is not None and all(v is not None and v >= least for v, least in zip(values, run_named(name)[0])))


def _stage(who, name, descend, *values):
    """The stage ``name`` bound to its options' values (pipeline.Stage.bind), or ``who``'s ValueError where ``stage_ok`` says no."""
    if not stage_ok(name, descend, *values):
        raise ValueError(f"ML2PN.{who}: {run_named(name)[1]}")
    from . import pipeline as pl
    return pl.stage_named(name).bind(*values)


def _stage_asked(who, descend, pair_rounds, pair_span=None, pair_rank=None):
    """``infer``'s and ``infer_services``' stage, ``stage_given``'s; the full pair sweep is ``infer``'s own and refused in its name."""
    name = stage_given(pair_rounds, pair_span, pair_rank)
    values = (pair_rounds, pair_span, pair_rank)[:len(RUNS[name][0])]
    return _stage(who if len(values) > 1 else "infer", name, descend, *values)


def search_plan(stage, multi):
    """How the test quarter goes through a (bound) stage, from every start (``multi``) or from the actions: the pipeline function, its
    keyword arguments beside max_sweeps, reduct and min_cost, the artefact, the per-problem fields of the result it lists and the
    settings beside them (no fields: the artefact has no ``extra``).  A pure function: no device is touched."""
    _, _, _, part, flag, written = run_named(stage.method)
    function, *names = stage.starts if multi else (stage.method, *stage.options)
    parts = [p for p in ("multistart" if multi else "", part) if p] or ["descent"]
    return (function, dict(zip(names, stage.values)), "ML+2PN+" + "+".join(parts) + ".txt", stage.row_keys + (flag,) if flag else (),
            {k: v for k, v in zip(written, stage.values) if k})


def _infer(dataset, net, low, high, n_per, epoch, device, batch_size, precision, woa, samples, sample_seed, descend, all_starts, stage,
           services=False):
    import torch
    from . import loadData as ld
    from .pipeline import DeviceBatch, DeviceServices, ML2PNPipeline
    if all_starts and (samples < 2 or descend is None):
        raise ValueError("ML2PN.infer: all_starts needs samples > 1 and descend")
    d = f"./data/{dataset}/"
    ds = {k: json.load(open(d + fn)) for k, fn in (
        ("nodefeatures", "nodefeatures.data"), ("edge_indices", "edge_indices.data"), ("labels", "labels.data"),
        ("serviceFeature", "serviceFeature.data"), ("minCostList", "minCostList.data"))}
    dev = torch.device(device)
    P = len(ds["nodefeatures"])
    T = len(ds["serviceFeature"])
    pipe = ML2PNPipeline(net.to(dev).eval(), low.to(dev).eval(), high.to(dev).eval(), n_per, precision=precision)
    table, _ = ld.tables_from_dataset(ds, 0, 0)
    svc = DeviceServices.from_table(table, dev)
    rankings, actions, test_actions, test_starts, test_ids = [], [[] for _ in range(T)], [], [], []      # (test_ids: ``services`` only)
    n_train = P // 4 * 3
    from . import ops
    for lo in range(0, P, batch_size):
        hi = min(P, lo + batch_size)
        _, pb = ld.tables_from_dataset(ds, lo, hi)
        batch = DeviceBatch.from_problems(pb, dev)
        # a timed-out inter-workgroup hand-off must never reach an artefact file: checked per batch, repeated once if it happens
        if samples > 1:
            seed_b = None if sample_seed is None else (int(sample_seed) + lo // batch_size) & 0x7FFFFFFFFFFFFFFF
            if seed_b is None:
                from .modelPN import fresh_seed
                seed_b = fresh_seed()           # one seed per batch
            # best_of checks its own launches before it returns: a failed hand-off raises there (no repeat of the batch)
            def best(attempt):
                o = pipe.best_of(svc, batch, samples, seed=seed_b, write_through=attempt > 0, return_all=all_starts)
                rows = o["actions_all"][..., -8:].cpu().numpy().astype(np.float64) if all_starts else None       # [b,N,T,8]
                ids = None
                if services:                    # the rows of the service table the action rows are: [b,T], with all_starts [b,N,T]
                    ids = o["candidate_ids"].gather(1, (o["idx_all"].flatten(1) if all_starts else o["idx_high"]).long()).cpu().numpy()
                    ids = ids.reshape(rows.shape[:3]) if all_starts else ids
                return o["actions"].cpu().numpy().astype(np.float64), rows, ids
            act, starts, ids = ops.run_checked(best, dev)
            if all_starts and hi > n_train:
                test_starts.append(starts[max(0, n_train - lo):])
        else:
            def one(attempt):
                o = pipe.run(svc, batch, write_through=attempt > 0)
                return (o["actions"].cpu().numpy().astype(np.float64),
                        o["candidate_ids"].gather(1, o["idx_high"].long()).cpu().numpy() if services else None)
            act, ids = ops.run_checked(one, dev)                             # [b,T,8], and (services) the rows of the service table they are [b,T]
        rankings += pipe.rankings(svc, batch).cpu().tolist()
        for b in range(hi - lo):
            if lo + b >= n_train:
                for t in range(T):
                    actions[t].append(act[b, t].tolist())
        if (woa is not None or descend is not None) and hi > n_train:
            test_actions.append(act[max(0, n_train - lo):])
            if services:
                test_ids.append(ids[max(0, n_train - lo):])
    paths = write_artifacts(dataset, epoch, rankings, actions)
    if woa is not None or descend is not None:
        _refine_test_quarter(dataset, ds, pipe, svc, np.concatenate(test_actions) if test_actions else np.zeros((0, T, 8)),
                            **(woa or {"popSize": 0, "MAX_Iter": 0, "reduct": 0}), descend=descend, stage=stage,
                            action_ids=np.concatenate(test_ids).astype(np.int32) if services and test_ids else None, services=services,
                            starts=(np.concatenate(test_starts) if test_starts else np.zeros((0, samples, T, 8))) if all_starts else None)
    return paths


def refine_test_quarter(dataset, ds, pipe, svc, actions, popSize, MAX_Iter, reduct, seed=None, descend=None, starts=None,
                        pair_rounds=None):
    """ES-WOA refinement of the test quarter's actions [nTest, T, 8] on the device, written as the WOA approach's
    ``ML+2PN+WOA.txt`` (WOA.py:286-296): quality = minCost / best fitness, problem ``idx`` on stream ``seed + idx``.
    ``descend`` = sweeps (>= 1): one-swap descent first, written as ``ML+2PN+descent.txt``; ES-WOA (popSize > 0) then starts from it.
    ``starts`` [nTest, N, T, 8] (with ``descend``): descent from every one of the N rows per problem, the lowest optimum kept
    (pipeline.descend_starts), written as ``ML+2PN+multistart.txt`` instead; ES-WOA then starts from the winner's rows.
    ``pair_rounds`` (>= 1, with ``descend``): pair-swap descent in place of the one-swap descent in each of these, written as
    ``ML+2PN+pairs.txt`` / ``ML+2PN+multistart+pairs.txt`` with the per-problem rounds, pair_moves and converged beside the four keys."""
    from . import pipeline as pl
    return _refine_test_quarter(dataset, ds, pipe, svc, actions, popSize, MAX_Iter, reduct, seed=seed, descend=descend, starts=starts,
                                stage=pl.ONE_SWAP if pair_rounds is None else pl.PAIRS.bind(pair_rounds))


def _refine_test_quarter(dataset, ds, pipe, svc, actions, popSize, MAX_Iter, reduct, seed=None, descend=None, starts=None, stage=None,
                         services=False, action_ids=None):
    """refine_test_quarter with any (bound) ``stage`` of pipeline.STAGES in the descent's place (with ``descend``): ``search_plan`` says
    which pipeline function runs it, from the actions or from ``starts``, into which file and with which ``extra``.  ES-WOA behind it
    starts from the one-swap descent or, where the stage has rounds, the full pair sweep with that many.
    ``services``: the last stage's compositions also go to ``ML+2PN+services.txt`` (write_services);
    ``action_ids`` [nTest, T] (with ``starts``: [nTest, N, T]) int32: the rows of the service table the action rows are, or None."""
    import time
    import torch
    from . import loadData as ld
    from .WOA import write_ml2pn_woa
    from . import pipeline as pl
    dev = svc.qos.device
    P = len(ds["nodefeatures"])
    first = P // 4 * 3
    n = actions.shape[0]
    _, pb = ld.tables_from_dataset(ds, first, first + n)
    batch = pl.DeviceBatch.from_problems(pb, dev)
    seeds = None if seed is None else [(seed + first + i) & 0xFFFFFFFFFFFFFFFF for i in range(n)]
    out = {"actions": torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float64)).to(dev)}
    min_cost = ds["minCostList"][first:first + n]
    written = None
    # each file books the time of its own stages: descent.txt the tables + descent, WOA.txt the tables (+ descent) + ES-WOA.  With
    # both, descent therefore runs twice (it is deterministic and costs about a hundredth of the ES-WOA run beside it).
    if descend is not None:
        multi = starts is not None                   # from every start or the actions
        function, options, name, fields, settings = search_plan(stage, multi)
        torch.cuda.synchronize(dev)
        t0 = time.time()
        res = getattr(pl, function)(svc, batch, torch.from_numpy(np.ascontiguousarray(starts, dtype=np.float64)).to(dev) if multi else out,
                                    max_sweeps=descend, reduct=reduct, min_cost=min_cost, **options)
        quality = res["quality"].cpu().tolist()
        extra = {**{k: res[k].cpu().tolist() for k in fields}, **settings} if fields else None
        written = write_ml2pn_woa(dataset, quality, (time.time() - t0) / max(n, 1), first, name=name, extra=extra)
        if multi:
            if services and action_ids is not None:  # the winner's ids, as its rows
                win = res["start_index"].long()[:, None, None]
                all_ids = torch.from_numpy(np.ascontiguousarray(action_ids)).to(dev)
                action_ids = all_ids.gather(1, win.expand(-1, 1, all_ids.shape[2]))[:, 0].cpu().numpy()
            out = {"actions": res["actions"]}        # refine below rebuilds the winner's tables and repeats its descent
    if descend is None or popSize > 0:
        torch.cuda.synchronize(dev)
        t0 = time.time()
        if descend is None:
            res = pipe.refine(svc, batch, out, popSize, MAX_Iter, reduct=reduct, seeds=seeds, min_cost=min_cost)
        else:
            res = pl.refine(svc, batch, out, popSize, MAX_Iter, reduct=reduct, seeds=seeds, min_cost=min_cost, descend=descend,
                            pair_rounds=dict(zip(stage.options, stage.values)).get("max_rounds", 0))
        quality = res["quality"].cpu().tolist()
        written = write_ml2pn_woa(dataset, quality, (time.time() - t0) / max(n, 1), first)
    if services:
        write_services(dataset, svc, batch, out, res, reduct, action_ids)
    return written


def write_services(dataset, svc, batch, out, res, reduct, action_ids=None):
    """``./solutions/WOA/<dataset>/ML+2PN+services.txt``: which services the compositions of the search result ``res`` over
    ``out["actions"]`` consist of (pipeline.name_services; ``action_ids`` [B, T]: the rows of the service table the actions are) and
    what pipeline.score_services says of them.  Per problem: ``services`` = the list of [node, category, service] of its task nodes (the node's
    position in its workflow graph, its 0-based category, the row of the service table or -1: no candidate list, or a foreign row
    without an id), ``merit``, ``best_fitness`` (the stage's own figure: equal to the merit bit for bit where every foreign row has an id),
    ``n_rows``.  json writes a float64 so that it reads back as the same bits."""
    import torch
    from . import pipeline as pl
    dev = svc.qos.device
    src = {"actions": out["actions"]}
    if action_ids is not None:                       # as name_services reads them off run's result: identity picks over the ids
        ids = torch.from_numpy(np.ascontiguousarray(action_ids, dtype=np.int32)).to(dev)
        src.update(candidate_ids=ids, idx_high=torch.arange(ids.shape[1], device=dev, dtype=torch.int32).expand(ids.shape[0], -1).contiguous())
    named = pl.name_services(svc, batch, src, {k: v for k, v in res.items() if k not in ("start_index", "actions")}, reduct=reduct)
    merit, n_rows = pl.score_services(svc, batch, named["node_services"])
    seg, x0 = batch.seg_ptr.cpu().tolist(), batch.x[:, 0].cpu().tolist()
    node = named["node_services"].cpu().tolist()
    fit = named["best_fitness"].cpu().tolist()
    rows = []
    for b in range(len(seg) - 1):
        rows.append([[g - seg[b], int(x0[g]) - 1, node[g]] for g in range(seg[b] + 1, seg[b + 1])])
    doc = {"services": rows, "merit": merit.cpu().tolist(), "best_fitness": fit, "n_rows": n_rows.cpu().tolist(),
           "action_ids_used": bool(named["action_ids_used"])}
    os.makedirs(f"./solutions/WOA/{dataset}/", exist_ok=True)
    with open(f"./solutions/WOA/{dataset}/ML+2PN+services.txt", "w") as f:
        json.dump(doc, f)
    return doc


def artifact_paths(dataset, epoch):
    """Where ``loadDataPN`` / ``check`` look (loadData.py:84-89, ML2PN.py:25-28): epoch -1 -> ./solutions/pretrained/."""
    if epoch == -1:
        return f"./solutions/pretrained/{dataset}-ML.txt", f"./solutions/pretrained/{dataset}-PNHigh.txt"
    return f"./solutions/ML/{dataset}/testServices-epoch{epoch}.txt", f"./solutions/PNHigh/{dataset}/allActions{epoch}.txt"


def write_artifacts(dataset, epoch, rankings, actions):
    """The two artefacts of an ML+2PN run in the reference's formats: rankings [P][S] ints as TrainML.start dumps them
    (trainML.py:146-149) and the High-level actions [T][nTest][8] floats as the PNHigh eval block dumps them
    (trainPNHigh.py:133-144)."""
    p_rank, p_act = artifact_paths(dataset, epoch)
    for p in (p_rank, p_act):
        os.makedirs(os.path.dirname(p), exist_ok=True)
    with open(p_rank, "w") as f:
        json.dump(rankings, f)
    with open(p_act, "w") as f:
        json.dump(actions, f)
    return p_rank, p_act

"""What the four search benches (bench_refine, bench_descend, bench_multistart, bench_pairs) share: the two configurations, the
generator of their start rows, the synthetic data set with its device tables and stream seeds, and the timing of one call."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {"qws": dict(T=47, S=2507, tasks=10, reduct=0, pop=50, iters=250),
           "normal": dict(T=50, S=5000, tasks=10, reduct=0.55, pop=60, iters=500)}


def _seed_rows(ds, reduct, g, foreign=0.1):
    """[nTest, T, 8] action rows: a member of every task's addS list (foreign rows now and then), dummies elsewhere."""
    from gnnpn_sc_amd.loadData import addS
    sf = ds["serviceFeature"]
    n_cat = len(sf)
    div, mod = [], []
    for key in sf:
        div += [int(key) - 1] * len(sf[key])
        mod += list(range(len(sf[key])))
    P = len(ds["nodefeatures"])
    n_train = P // 4 * 3
    acts = np.zeros((P - n_train, n_cat, 8))
    acts[:, :, 1:4] = 1.0
    for b, nodes in enumerate(ds["nodefeatures"][n_train:]):
        cons = {c: [0] * 8 for c in range(1, n_cat + 1)}
        for node in nodes:
            pair = node[-5:-3] + node[-2:]
            if node[0] == 1:
                for c in cons:
                    cons[c][-4:] = pair
            else:
                cons[node[:-6].index(1)][-8:-4] = pair
        cats = [n[:-6].index(1) - 1 for n in nodes][1:]
        for c, lst in zip(cats, addS(range(len(div)), sf, cons, cats, div, mod, reduct, None)):
            if lst:
                acts[b, c, :4] = np.r_[g.random(2), 0.9 + 0.1 * g.random(2)] if g.random() < foreign else lst[int(g.integers(0, len(lst)))]
    return acts


def dataset(cfg, n_test):
    """The synthetic data set whose test quarter has ``n_test`` problems (seed 1)."""
    import gnnpn_sc_amd.synth as synth
    return synth.make_dataset(cfg["T"], cfg["S"], n_test * 4, seed=1, tasks_per_problem=cfg["tasks"])


def setup(cfg, n_test, dev, last=None, ds=None):
    """(data set, services, batch, first, seeds) of the test quarter of ``dataset(cfg, n_test)`` (``ds``: that data set, where the
    caller has it already) on ``dev``: problems first .. first + last of it (``last`` None: all n_test), stream seeds
    1000 + first + i as an int64 device tensor."""
    import torch
    from gnnpn_sc_amd.loadData import tables_from_dataset
    from gnnpn_sc_amd.pipeline import DeviceBatch, DeviceServices
    ds = dataset(cfg, n_test) if ds is None else ds
    first = len(ds["nodefeatures"]) // 4 * 3
    table, pb = tables_from_dataset(ds, first, None if last is None else first + last)
    seeds = torch.tensor([1000 + first + i for i in range(n_test if last is None else last)], dtype=torch.int64, device=dev)
    return ds, DeviceServices.from_table(table, dev), DeviceBatch.from_problems(pb, dev), first, seeds


def timed(fn, dev):
    """(fn(), its milliseconds between two HIP events)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return out, e0.elapsed_time(e1)


def mean(t):
    return round(float(t.double().mean().item()), 6)


def share(t):
    return round(float(t.double().mean().item()), 4)

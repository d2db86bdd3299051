"""Device-resident end-to-end ML+2PN inference: what the reference spreads over
``TrainML.test`` (/root/reference/src/models/trainML.py:49-72) -> JSON -> ``loadDataPN``
(src/loadData.py:72-152) -> JSON -> the eval block of ``TrainModel.train_and_validate``
(src/models/trainPNHigh.py:131-150), as one stream of kernels with nothing leaving HBM between
the stages:

    GNN scores [B,S] -> per-category top-K feasible candidates -> PN input rows [B,L,8]
    -> Low/High encoders (one launch) -> Low decode -> High decode -> QoS reward

Inputs are ``DeviceBatch``/``DeviceServices`` (packed once from the host structures of synth.py /
loadData.py); outputs stay on the device.
"""
import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, custom_ops, graph, ops, score_plan   # noqa: F401  (custom_ops registers torch.ops.gnnpn.*)
from .modelPN import two_level_best_of, two_level_greedy


@dataclass
class DeviceServices:
    """Problem-independent service side, resident in HBM."""
    x_service: torch.Tensor      # f32 [S,5]
    csr: graph.CSR               # self-loop-complete destination-major CSR, raw weights
    cat_ptr: torch.Tensor        # i32 [T+1]
    qos: torch.Tensor            # f64 [S,4]
    emb_cache: tuple = None      # (prepared-weights object, [S,hidden] service embedding): see ML2PNPipeline.service_embedding
    score_cache: score_plan.OperandCache = None   # the fused score + select kernel's operands for emb_cache's embedding: see ML2PNPipeline.score_select_operands

    @staticmethod
    def from_table(table, device):
        ei = torch.from_numpy(np.ascontiguousarray(table.edge_index))
        ea = torch.from_numpy(np.ascontiguousarray(table.edge_attr))
        csr = graph.gcn_csr(ei, ea, table.n_services).to(device)
        return DeviceServices(torch.from_numpy(table.x_service).to(device), csr,
                              torch.from_numpy(np.ascontiguousarray(table.cat_ptr)).to(device),
                              torch.from_numpy(np.ascontiguousarray(table.qos)).to(device))


@dataclass
class DeviceBatch:
    """B composition requests, resident in HBM."""
    x: torch.Tensor              # f32 [N,7]
    wf_csr: graph.CSR
    seg_ptr: torch.Tensor        # i32 [B+1]
    local_bounds: torch.Tensor   # f64 [B,T,4]
    present: torch.Tensor        # u8  [B,T]
    global_bounds: torch.Tensor  # f64 [B,4]
    max_nodes: int = 0           # > 0: every workflow graph has at most this many nodes AND every edge stays inside its
    #                              graph (host-checked when the batch was packed) -> the one-launch GIN branch may be used

    @property
    def n_problems(self):
        return self.present.shape[0]

    @staticmethod
    def from_problems(pb, device):
        ei = torch.from_numpy(np.ascontiguousarray(pb.edge_index))
        batch = torch.from_numpy(np.ascontiguousarray(pb.batch))
        n = pb.x.shape[0]
        inside = bool((pb.batch[pb.edge_index[0]] == pb.batch[pb.edge_index[1]]).all()) if pb.edge_index.size else True
        max_nodes = int(np.bincount(pb.batch, minlength=1).max()) if inside and n else 0
        return DeviceBatch(torch.from_numpy(pb.x).to(device), graph.csr_by_destination(ei, n).to(device),
                           graph.segment_ptr(batch, pb.n_problems).to(device),
                           torch.from_numpy(np.ascontiguousarray(pb.local_bounds)).to(device),
                           torch.from_numpy(np.ascontiguousarray(pb.present)).to(device),
                           torch.from_numpy(np.ascontiguousarray(pb.global_bounds)).to(device), max_nodes)

    def shard(self, rank, world):
        """Contiguous shard of the problems for one rank (dist.py); graphs stay whole."""
        B = self.n_problems
        lo, hi = B * rank // world, B * (rank + 1) // world
        seg = self.seg_ptr.cpu()
        n0, n1 = int(seg[lo]), int(seg[hi])
        rp = self.wf_csr.rowptr.cpu()
        e0, e1 = int(rp[n0]), int(rp[n1])
        dev = self.x.device
        csr = graph.CSR((rp[n0:n1 + 1] - e0).to(dev), (self.wf_csr.col[e0:e1] - n0).contiguous(), None, n1 - n0)
        return DeviceBatch(self.x[n0:n1].contiguous(), csr, (seg[lo:hi + 1] - n0).to(dev),
                           self.local_bounds[lo:hi].contiguous(), self.present[lo:hi].contiguous(),
                           self.global_bounds[lo:hi].contiguous(), self.max_nodes)


# Hand-off form of the cooperative kernels in the runner's launches (gnnpn_launch_opts_t.write_through): False = granule stores
# that stay in the group's XCD L2 (faster; correct by this toolchain's lowering and by the run-time XCD placement of a group),
# True = agent-scope write-through stores (valid by the HIP memory model, placement independent).  What can go wrong with the
# fast form is liveness, not data: a granule is ONE 8-byte store carrying its own tag, so a reader sees an old granule or a new
# one, never a mixture — a store that does not become visible ends in a bounded-spin time-out (status 1 / 2), and a launch that
# did not run at all in a shortfall of finished workgroup-tiles (status 16): both are loud at the next poll / synchronize, and
# the runner then switches ITSELF to the write-through form for the rest of its life (``auto_degrade``).  DESIGN.md sections 4.5-4.6.
DEFAULT_WRITE_THROUGH = os.environ.get("GNNPN_PIPE_WRITE_THROUGH", "0") == "1"
HOST_COPY_ON_ITS_OWN_STREAM = os.environ.get("GNNPN_HOST_COPY_INLINE") != "1"
COMMON_START_US = 0.0       # PipelinedRunner: > 0 holds the first replays of a burst until both are enqueued, at most this long.  OPT-IN since
#                             round 5 (GNNPN_PIPE_COMMON_START_US=400 is what round 4 ran): the slots no longer slip apart once the front-half
#                             kernels share the cooperative kernels' LDS footprint (FRONT_LDS_KB below), which is also 1 % faster than the gate


def half_batch_split(n_problems):
    """Where a batch is cut for the two half-batches that run side by side: whole tiles of 16 problems to the first half,
    the (possibly ragged) rest to the second; 0 when there is nothing to put on the second stream."""
    half = ((int(n_problems) + 31) // 32) * 16
    return half if 0 < half < n_problems else 0


_warned_partitioned = set()


def warn_partitioned_device(device, precision):
    """Say ONCE per device what a compute-partitioned GPU means for this path.  The cooperative recurrent
    kernels — the ones every measured number of this package comes from — are placed for 8 XCDs x 32 CUs (MI355X in SPX mode:
    csrc/coop_common.h::coop_place deals seats per XCD and assumes eight of them).  On a device that shows fewer than 256 compute
    units (CPX / DPX / QPX partitions, or another GPU) their launchers return GNNPN_E_UNSUP: with precision "split" or "f16" the
    recurrent calls then RAISE; with "f32" the decoder in auto mode (impl 0) takes the per-workgroup streaming form and the encoder
    raises unless impl=1 is passed — the streaming forms re-stream the 1 MiB W_hh from L2 every step, about 10 x slower per step
    (11 us against 2.4 us / 3.2 us at the QWS shape, csrc/lstm_coop.hip)."""
    import warnings
    if device.type != "cuda":
        return
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _warned_partitioned:
        return
    _warned_partitioned.add(idx)
    n_cu = torch.cuda.get_device_properties(idx).multi_processor_count
    if n_cu < 256:
        warnings.warn(f"gnnpn: cuda:{idx} shows {n_cu} compute units; the cooperative recurrent kernels are built for 8 XCDs x 32 CUs (MI355X, SPX "
                      f"mode). precision={precision!r}: " + ("the recurrent launches will raise GNNPN_E_UNSUP — " if precision != "f32" else "") +
                      "only the per-workgroup streaming forms (precision='f32', impl=1) run here, about 10 x slower per recurrent step.",
                      RuntimeWarning, stacklevel=3)


def _quality(res, min_cost, dev):
    """quality = min_cost / best_fitness (WOA.py:286-287), added to ``res`` where ``min_cost`` [B] is given."""
    if min_cost is not None:
        mc = min_cost if isinstance(min_cost, torch.Tensor) else torch.as_tensor(np.asarray(min_cost, dtype=np.float64))
        res["quality"] = mc.to(device=dev, dtype=torch.float64) / res["best_fitness"]
    return res


class Stage(NamedTuple):
    """One search stage over candidate tables, written down once: what every layer above ``ops`` needs to know of it."""
    method: str                  # the SearchTables method that runs it — and the name of the public function of one start per problem
    options: tuple               # its option names, in the method's call order behind max_sweeps
    refusal: str                 # what a negative option is told
    starts: tuple                # the ``descend_starts*`` function that runs it from every start, and the options that one takes, in order
    lane_only: bool = False      # it has the lane form only: at most 64 slots per problem
    row_keys: tuple = ()         # its per-row [B * N] fields that ``_descend_starts`` also keeps per start, [B, N], as ``<key>_all``
    winner_rows: tuple = ()      # its per-row [B * N, n] fields of which ``_descend_starts`` keeps the winner's row
    values: tuple = ()           # a bound stage (``bind``): its options' values, ints

    def bind(self, *values, who=None):
        """This stage with its options' values, refused where one is negative (``who``: the public name that says so, where it is
        not ``method``)."""
        if min((int(v) for v in values), default=0) < 0:
            raise ops.GnnpnError(f"{who or self.method}: " + self.refusal.format(*values))
        return self._replace(values=tuple(int(v) for v in values))


# The five stages: one-swap descent, pair-swap descent under its three public names, the tabu walk.
STAGES = {s.method: s for s in (
    Stage("descend", (), "", ("descend_starts",)),
    Stage("descend_pairs", ("max_rounds",), "the number of rounds must be >= 0, got {}", ("descend_starts_pairs", "pair_rounds"),
          lane_only=True, row_keys=("rounds", "pair_moves")),
    Stage("descend_pairs_windowed", ("max_rounds", "max_span"), "the number of rounds and the span must be >= 0, got {} and {}",
          ("descend_starts_pairs", "pair_rounds"), row_keys=("rounds", "pair_moves")),     # (from every start: the full sweep, no span)
    Stage("descend_pairs_shortlist", ("max_rounds", "max_span", "max_rank"),
          "the number of rounds, the span and the rank must be >= 0, got {}, {} and {}",
          ("descend_starts_pairs_shortlist", "pair_rounds", "pair_span", "pair_rank"), row_keys=("rounds", "pair_moves")),
    Stage("descend_tabu", ("max_steps", "tenure"), "the number of steps and the tenure must be >= 0, got {} and {}",
          ("descend_starts_tabu", "max_steps", "tenure"), row_keys=("steps", "best_step"), winner_rows=("walk",)))}
ONE_SWAP, PAIRS, PAIRS_WINDOWED, PAIRS_SHORTLIST, TABU = STAGES.values()

# The stages added since: the tabu walk over pair moves.  A table of its own beside STAGES, whose five rows the host tests pin by name;
# ``stage_named`` reads both.
MORE_STAGES = {s.method: s for s in (
    Stage("descend_tabu_pairs", ("max_steps", "tenure", "max_rank", "max_span"),
          "the number of steps, the tenure, the rank and the span must be >= 0, got {}, {}, {} and {}",
          ("descend_starts_tabu_pairs", "max_steps", "tenure", "max_rank", "max_span"), row_keys=("steps", "best_step", "pair_steps"),
          winner_rows=("walk",)),)}
(TABU_PAIRS,) = MORE_STAGES.values()


def stage_named(name):
    """The stage of that method name: STAGES' first, then MORE_STAGES'."""
    return STAGES[name] if name in STAGES else MORE_STAGES[name]


def _search_tables(tabs, max_sweeps, stage=ONE_SWAP):
    """The (bound) stage over the tables; plus n_slots."""
    if stage.lane_only and tabs["max_slots"] > 64:
        raise ops.GnnpnError(f"{stage.method}: a problem of the batch has {tabs['max_slots']} slots; the pair sweep takes at most 64 "
                             "per problem (descend runs one-swap descent at any slot count)")
    res = getattr(tabs, stage.method)(max_sweeps, *stage.values)
    res["n_slots"] = tabs["n_slots"]
    return res


def _descend_tables(tabs, max_sweeps, pair_rounds=None):
    """One-swap descent over the tables, or (pair_rounds an int, 0 included) ``descend_pairs`` with that many rounds allowed."""
    return _search_tables(tabs, max_sweeps, ONE_SWAP if pair_rounds is None else PAIRS.bind(pair_rounds))


def _descend_actions(services, batch, out, max_sweeps, stage, reduct, min_cost, patches):
    """``descend``, the three ``descend_pairs*``, ``descend_tabu`` and ``descend_tabu_pairs``: the tables of ``out["actions"]``, the (bound) stage over them,
    the quality."""
    actions = out["actions"]
    tabs = ops.woa_candidates(services.cat_ptr, services.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds,
                              actions, reduct=reduct, patches=patches)
    return _quality(_search_tables(tabs, max_sweeps, stage), min_cost, actions.device)


@torch.no_grad()
def descend(services, batch, out, max_sweeps=16, reduct=0, min_cost=None, patches=()):
    """One-swap descent of ``out["actions"]`` on the device: the candidate lists of every problem as ``refine`` builds them
    (gnnpn_woa_candidates_count / _fill), then per problem, slot by slot, the best candidate of the slot's list while it
    strictly lowers violate + objFunc, until a sweep moves nothing or ``max_sweeps`` are done (gnnpn_descend_ragged_f64; all
    problems in one launch, deterministic: no seeds).  A problem the host path raises on raises GnnpnError naming it.
    ``ML2PNPipeline.descend`` is this, as a method.  Returns ops.descend_ragged's dict (best_fitness, start_fitness, best_pos,
    best_rows, history, sweeps, moves) plus n_slots [B] i32 (and quality [B] f64 = min_cost / best_fitness)."""
    return _descend_actions(services, batch, out, max_sweeps, ONE_SWAP, reduct, min_cost, patches)


@torch.no_grad()
def descend_pairs(services, batch, out, max_sweeps=16, max_rounds=4, reduct=0, min_cost=None, patches=()):
    """Pair-swap descent of ``out["actions"]`` on the device: ``descend``'s tables and one-swap descent, then up to ``max_rounds``
    rounds of one pair sweep (every two slots, every pair of their candidates, the best taken while it strictly lowers violate +
    objFunc) and the one-swap descent again (gnnpn_descend_pairs_ragged_f64; all problems in one launch, deterministic).  It leaves
    the one-swap optima behind a +1 wall: a swap that breaks a product bound which a second swap restores.  At most 64 slots per
    problem: a larger one raises GnnpnError (``descend`` takes any).  ``ML2PNPipeline.descend_pairs`` is this, as a method.  Returns
    ops.descend_pairs_ragged's dict (best_fitness, start_fitness, best_pos, best_rows, round_history, sweeps, moves, rounds,
    pair_moves, converged) plus n_slots [B] i32 (and quality [B] f64 = min_cost / best_fitness).  ``max_rounds`` = 0: ``descend``'s
    result in every shared field."""
    return _descend_actions(services, batch, out, max_sweeps, PAIRS.bind(max_rounds), reduct, min_cost, patches)


@torch.no_grad()
def descend_pairs_windowed(services, batch, out, max_sweeps=16, max_rounds=4, max_span=0, reduct=0, min_cost=None, patches=()):
    """``descend_pairs`` at any slot count and over a window of neighbouring slots (gnnpn_descend_pairs_windowed_ragged_f64): the same
    tables, the same search, the same dict.  ``max_span`` = 0: every slot pair; s > 0: only slots at most s apart, which is what
    makes a pair sweep affordable at hundreds of slots (converged then means: no single swap and no pair within the span lowers the
    result).  Problems of more than 64 slots run in the workgroup form (all of the batch, then).  A negative span or a negative
    number of rounds raises GnnpnError.  ``ML2PNPipeline.descend_pairs_windowed`` is this, as a method."""
    return _descend_actions(services, batch, out, max_sweeps, PAIRS_WINDOWED.bind(max_rounds, max_span), reduct, min_cost, patches)


@torch.no_grad()
def descend_pairs_shortlist(services, batch, out, max_sweeps=16, max_rounds=4, max_span=0, max_rank=0, reduct=0, min_cost=None, patches=()):
    """``descend_pairs_windowed`` whose pair sweeps look only at the ``max_rank`` best candidates of each slot
    (gnnpn_descend_pairs_shortlist_ragged_f64): the same tables, the same dict.  ``max_rank`` = 0: no shortlist, that function's
    result.  m > 0: before every pair sweep each slot keeps the m candidates whose single swap into the current composition has the
    lowest merit, so a slot pair costs at most m * m evaluations (converged then means: no single swap, and no pair within the span
    and the final composition's shortlists, lowers the result).  Any slot count.  A negative span, rank or number of rounds raises
    GnnpnError.  ``ML2PNPipeline.descend_pairs_shortlist`` is this, as a method."""
    return _descend_actions(services, batch, out, max_sweeps, PAIRS_SHORTLIST.bind(max_rounds, max_span, max_rank), reduct, min_cost, patches)


@torch.no_grad()
def descend_tabu(services, batch, out, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, reduct=0, min_cost=None, patches=()):
    """Tabu walk of ``out["actions"]`` on the device (gnnpn_descend_tabu_ragged_f64; all problems in one launch, deterministic: no
    seeds): ``descend``'s tables and one-swap descent, then up to ``max_steps`` steps that each take the best single swap of the
    composition whether or not it lowers violate + objFunc, the position a slot leaves barred for ``tenure`` steps unless the swap
    beats the best merit seen; the best composition seen is the result (polished by the one-swap sweeps where the walk was cut at
    it).  It leaves one-swap optima that take several coordinated swaps to leave.  Any slot count.  A negative number of steps or
    tenure raises GnnpnError.  ``ML2PNPipeline.descend_tabu`` is this, as a method.  Returns ops.descend_tabu_ragged's dict
    (``descend``'s keys, history per step, walk, steps, best_step, stalled) plus n_slots [B] i32 (and quality [B] f64).
    ``max_steps`` = 0: ``descend``'s result in every shared field."""
    return _descend_actions(services, batch, out, max_sweeps, TABU.bind(max_steps, tenure), reduct, min_cost, patches)


@torch.no_grad()
def descend_starts_tabu(services, batch, starts, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, reduct=0, min_cost=None,
                        patches=()):
    """``descend_starts`` whose B * N rows go through the tabu walk (gnnpn_descend_tabu_ragged_f64 in place of the descent launch);
    the same selection (gnnpn_descend_select_f64, unchanged) picks the winner: history is the winner's walk history, steps,
    best_step and stalled [B] i32 and walk [B, max_steps] f64 are the winner's (gathered by start_index), steps_all and
    best_step_all are [B, N] i32.  ``max_steps`` = 0 is ``descend_starts``' result in every shared field.  A negative number of
    steps or tenure raises GnnpnError.  ``ML2PNPipeline.descend_starts_tabu`` is this, as a method."""
    return _descend_starts(services, batch, starts, max_sweeps, reduct, min_cost, patches,
                           TABU.bind(max_steps, tenure, who="descend_starts_tabu"))


@torch.no_grad()
def descend_tabu_pairs(services, batch, out, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, max_rank=ops.DEFAULT_PAIR_RANK, max_span=0,
                       reduct=0, min_cost=None, patches=()):
    """Tabu walk over pair moves of ``out["actions"]`` on the device (gnnpn_descend_tabu_pairs_ragged_f64; all problems in one launch,
    deterministic: no seeds): ``descend_tabu`` whose step takes the best admissible single swap or pair swap — a pair exchanges two
    slots (``max_span`` = s > 0: at most s apart) for candidates of their shortlists, the ``max_rank`` best single swaps of each
    slot, formed anew every step (0: whole lists).  It crosses in one step a product-bound wall that costs the tabu walk two, and
    goes on past the pair optimum at which the pair sweeps stop.  Any slot count.  A negative number of steps, tenure, rank or span
    raises GnnpnError.  ``ML2PNPipeline.descend_tabu_pairs`` is this, as a method.  Returns ops.descend_tabu_pairs_ragged's dict
    (``descend_tabu``'s keys plus pair_steps) plus n_slots [B] i32 (and quality [B] f64).  ``max_steps`` = 0: ``descend``'s result
    in every shared field."""
    return _descend_actions(services, batch, out, max_sweeps, TABU_PAIRS.bind(max_steps, tenure, max_rank, max_span), reduct, min_cost, patches)


@torch.no_grad()
def descend_starts_tabu_pairs(services, batch, starts, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, max_rank=ops.DEFAULT_PAIR_RANK,
                              max_span=0, reduct=0, min_cost=None, patches=()):
    """``descend_starts`` whose B * N rows go through the tabu walk over pair moves (gnnpn_descend_tabu_pairs_ragged_f64 in place of
    the descent launch); the same selection (gnnpn_descend_select_f64, unchanged) picks the winner: ``descend_starts_tabu``'s result
    plus pair_steps [B] i32 (the winner's) and pair_steps_all [B, N] i32.  A negative number of steps, tenure, rank or span raises
    GnnpnError.  ``ML2PNPipeline.descend_starts_tabu_pairs`` is this, as a method."""
    return _descend_starts(services, batch, starts, max_sweeps, reduct, min_cost, patches,
                           TABU_PAIRS.bind(max_steps, tenure, max_rank, max_span, who="descend_starts_tabu_pairs"))


@torch.no_grad()
def descend_starts(services, batch, starts, max_sweeps=16, reduct=0, min_cost=None, patches=()):
    """Multi-start descent: ``descend`` from N start compositions per problem, the lowest local optimum kept.  ``starts``: a
    [B, N, T', 8|9] tensor (float32 or float64) or a mapping with ``actions_all`` (what ``best_of(..., return_all=True)`` returns);
    the last 8 columns are used.  Three stages, all B * N (problem, replica) rows in each launch: the candidate tables of every
    row (gnnpn_woa_candidates_replicas_count / _fill — per replica, because with reduct != 0 the lists depend on the pick set and
    a foreign pick is appended per replica), one gnnpn_descend_ragged_f64 over the rows, and the selection
    (gnnpn_descend_select_f64: the smallest best_fitness, the lowest replica among equals, a NaN never).  Deterministic: no seeds.
    A row the host path raises on raises GnnpnError naming problem and replica.  ``ML2PNPipeline.descend_starts`` is this, as a
    method.  Returns ``descend``'s keys for the winners plus start_index [B] i32, actions [B, T', 8] (the winner's start rows:
    ``refine(services, batch, res, ..., descend=k)`` rebuilds its tables and repeats its descent before ES-WOA), fitness_all and
    start_fitness_all [B, N] f64, sweeps_all and moves_all [B, N] i32 (and quality [B] f64 = min_cost / best_fitness)."""
    return _descend_starts(services, batch, starts, max_sweeps, reduct, min_cost, patches, ONE_SWAP)


@torch.no_grad()
def descend_starts_pairs(services, batch, starts, max_sweeps=16, pair_rounds=4, reduct=0, min_cost=None, patches=()):
    """``descend_starts`` with pair-swap descent per row.  ``pair_rounds`` = r > 0: the B * N rows go through pair-swap descent
    with r rounds allowed (gnnpn_descend_pairs_ragged_f64 in place of the descent launch; at most 64 slots per problem); the
    same selection (gnnpn_descend_select_f64, unchanged) picks the winner, the result has round_history in place of history and
    gains rounds, pair_moves and converged [B] i32 (the winner's, gathered by start_index) and rounds_all, pair_moves_all [B, N] i32.
    ``pair_rounds`` = 0 is ``descend_starts``: the same launches, the same result.  ``descend_starts`` itself keeps its
    signature, which is why this is a function of its own.  ``ML2PNPipeline.descend_starts_pairs`` is this, as a method."""
    return _descend_starts(services, batch, starts, max_sweeps, reduct, min_cost, patches,
                           PAIRS.bind(pair_rounds) if int(pair_rounds) else ONE_SWAP)


@torch.no_grad()
def descend_starts_pairs_shortlist(services, batch, starts, max_sweeps=16, pair_rounds=4, pair_span=0, pair_rank=0, reduct=0, min_cost=None,
                                   patches=()):
    """``descend_starts_pairs`` whose B * N rows go through gnnpn_descend_pairs_shortlist_ragged_f64: any slot count, only slots at
    most ``pair_span`` apart (0: every pair) and only the ``pair_rank`` best candidates of each slot (0: all) — what makes pair-swap
    descent affordable N times over; the same selection (gnnpn_descend_select_f64, unchanged) picks the winner.  ``pair_span`` =
    ``pair_rank`` = 0 at up to 64 slots is ``descend_starts_pairs``' result in every shared field (``pair_rounds`` = 0 included: then
    the rows' one-swap descent, reported in the pair-swap format).  A negative span, rank or number of rounds raises GnnpnError.
    ``ML2PNPipeline.descend_starts_pairs_shortlist`` is this, as a method."""
    return _descend_starts(services, batch, starts, max_sweeps, reduct, min_cost, patches,
                           PAIRS_SHORTLIST.bind(pair_rounds, pair_span, pair_rank, who="descend_starts_pairs_shortlist"))


def _descend_starts(services, batch, starts, max_sweeps, reduct, min_cost, patches, stage):
    """The ``descend_starts*``: the tables of every start, the (bound) stage over them, the selection, the per-start fields
    (the stage's own among them), the quality."""
    all_rows = starts["actions_all"] if hasattr(starts, "keys") else starts
    if not isinstance(all_rows, torch.Tensor) or all_rows.dim() != 4 or all_rows.shape[3] not in (8, 9):
        raise ops.GnnpnError(f"descend_starts: starts [B, N, T, 8|9] expected, got {tuple(getattr(all_rows, 'shape', ()))}")
    all_rows = all_rows[..., -8:].contiguous()
    B, N = all_rows.shape[:2]
    tabs = ops.woa_candidates_replicas(services.cat_ptr, services.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds,
                                       all_rows, reduct=reduct, patches=patches)
    per_row = _search_tables(tabs, max_sweeps, stage)
    res = ops.descend_select(per_row, all_rows, tabs["n_slots"])        # (the rounds' merits and counters too, where there are any)
    res.update(fitness_all=per_row["best_fitness"].view(B, N), start_fitness_all=per_row["start_fitness"].view(B, N),
               sweeps_all=per_row["sweeps"].view(B, N), moves_all=per_row["moves"].view(B, N))
    res.update({k + "_all": per_row[k].view(B, N) for k in stage.row_keys})
    for k in stage.winner_rows:
        rows = per_row[k].reshape(B, N, -1)
        res[k] = rows.gather(1, res["start_index"].long()[:, None, None].expand(B, 1, rows.shape[2]))[:, 0]
    return _quality(res, min_cost, all_rows.device)


@torch.no_grad()
def refine(services, batch, out, popSize, MAX_Iter, reduct=0, seeds=None, min_cost=None, patches=(), descend=0, pair_rounds=0):
    """The third stage: ES-WOA refinement of ``out["actions"]`` (what ``run`` returned, or any mapping with an actions
    tensor [B,T,8], float32 or float64) on the device — the candidate lists of every problem built from ``services`` /
    ``batch`` (gnnpn_woa_candidates_count / _fill: loadDataOther + WOA._prepare, bit for bit) and the search of every problem
    in one launch (gnnpn_eswoa_ragged_f64: WOA.fine_tune).  ``seeds``: [B] stream seeds (None: fresh OS entropy, as
    fine_tune); ``min_cost`` [B]: adds quality = min_cost / best_fitness (WOA.py:286-287); ``patches``: WOA._prepare's.
    A problem the host path raises on raises GnnpnError naming it.  ``ML2PNPipeline.refine`` is this, as a method.
    Returns device tensors: best_fitness [B] f64, best_rows [B, max_slots, 4] f64, n_slots [B] i32, best_pos
    [B, max_slots] i32 (negative: Python list positions), history [B, MAX_Iter] f64, draws [B] i64 (and quality [B] f64).
    ``descend`` = k > 0: the tables are built once, one-swap descent runs up to k sweeps on them (``descend`` above) and ES-WOA
    starts from descent's best_pos in place of start_pos; the result gains ``descent`` (the descent's dict).  ``pair_rounds`` = r > 0
    (with or without ``descend``, which then allows 0 sweeps): pair-swap descent with r rounds allowed in place of the one-swap
    descent (``descend_pairs``), ``descent`` is its dict."""
    actions = out["actions"]
    dev = actions.device
    B = batch.n_problems
    tabs = ops.woa_candidates(services.cat_ptr, services.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds,
                              actions, reduct=reduct, patches=patches)
    if seeds is None:
        seeds = np.frombuffer(os.urandom(8 * B), dtype=np.int64).copy()
    if not isinstance(seeds, torch.Tensor):
        seeds = torch.from_numpy(np.asarray(seeds, dtype=np.uint64).reshape(B).view(np.int64).copy())
    seeds = seeds.to(device=dev, dtype=torch.int64).contiguous()
    start_pos, descent = None, None
    if descend or pair_rounds:
        descent = _quality(_descend_tables(tabs, int(descend), int(pair_rounds) if pair_rounds else None), min_cost, dev)
        start_pos = tabs.flat(descent["best_pos"])
    fit, pos, hist, draws, rows = tabs.eswoa(popSize, MAX_Iter, seeds, start_pos)
    res = {"best_fitness": fit, "best_rows": rows, "n_slots": tabs["n_slots"], "best_pos": pos, "history": hist, "draws": draws}
    if descent is not None:
        res["descent"] = descent
    return _quality(res, min_cost, dev)


def action_ids_of(out):
    """The rows of the service table that ``out["actions"]`` are, [B, T] i32, where ``out`` is ``run``'s or ``best_of``'s result:
    candidate_ids (select.hip writes the row ``s`` of ``qos`` a candidate was read from, -1 for a dummy row) gathered by idx_high
    (the decoder's picks, positions in the candidate sequence).  None where ``out`` does not carry both."""
    if not hasattr(out, "keys") or "candidate_ids" not in out or "idx_high" not in out:
        return None
    return out["candidate_ids"].gather(1, out["idx_high"].long()).to(torch.int32).contiguous()


def _start_action_ids(starts, start_index):
    """action_ids_of for the winning start of a multi-start result: idx_all [B, N, T] (``best_of(..., return_all=True)``) read at
    start_index in idx_high's place.  None where ``starts`` does not carry it."""
    if not hasattr(starts, "keys") or "candidate_ids" not in starts or "idx_all" not in starts:
        return None
    idx_all = starts["idx_all"]
    idx = idx_all.gather(1, start_index.long()[:, None, None].expand(-1, 1, idx_all.shape[2]))[:, 0]
    return starts["candidate_ids"].gather(1, idx.long()).to(torch.int32).contiguous()


@torch.no_grad()
def name_services(services, batch, out, res, reduct=0, patches=()):
    """Which services the composition of a search result consists of.  ``res``: what ``descend``, the three ``descend_pairs*``,
    the three ``descend_starts*`` or ``refine`` returned for ``out`` with the same ``reduct`` and ``patches``.  The tables are
    rebuilt with their ids (ops.woa_candidates_named: deterministic, the tables the search ran on) — of ``res["actions"]`` for a
    multi-start result (the winner's start rows), else of ``out["actions"]`` — and ``res["best_pos"]`` is mapped through them
    (gnnpn_search_services; ``refine``'s positions are ES-WOA's, negative ones Python's).  Where ``out`` carries candidate_ids and
    idx_high (``run``'s result; for a multi-start result idx_all, read at the winner), an appended foreign row is named by
    ``action_ids_of(out)``; else foreign rows are -1.  Returns ``res``'s keys plus best_services [B, max_slots] i32, node_services [N] i32 (one entry per row
    of batch.x, -1 where the node has no service) and action_ids_used (a bool).  An id s >= 0 means: row s of the service table,
    rounded where the tables were seeded, equals best_rows there, absent a patch on that row."""
    multi = "start_index" in res and "actions" in res
    actions = res["actions"] if multi else out["actions"]
    ids = _start_action_ids(out, res["start_index"]) if multi else action_ids_of(out)
    tabs = ops.woa_candidates_named(services.cat_ptr, services.qos, batch.x, batch.seg_ptr, batch.local_bounds, batch.global_bounds,
                                    actions, reduct=reduct, patches=patches, action_ids=ids)
    named = tabs.services(res, batch.seg_ptr, batch.x.shape[0])
    return {**res, **named, "action_ids_used": ids is not None}


@torch.no_grad()
def score_services(services, batch, node_services, rounded=True):
    """The figure of merit (violate + objFunc under the batch's global bounds) of compositions given as service ids, one entry of
    ``node_services`` per row of batch.x (-1: no service): ops.services_merit over the service table.  ``rounded``: the rows go
    through round(v, 5), as the tables of a search that started from action rows hold them — then scoring ``name_services``'
    node_services gives that search's best_fitness bit for bit (no patches; foreign rows named).  Returns (merit [B] f64,
    n_rows [B] i32)."""
    return ops.services_merit(batch.seg_ptr, node_services, services.qos, batch.global_bounds, rounded)


class ML2PNPipeline:
    """net: modelML.Net; low/high: modelPN.CombinatorialRL (levels "Low"/"High")."""

    def name_services(self, services, batch, out, res, reduct=0, patches=()):
        """Module-level ``name_services`` (it needs no network)."""
        return name_services(services, batch, out, res, reduct=reduct, patches=patches)

    def __init__(self, net, low, high, n_per, precision=None):
        from .modelPN import default_precision
        self.net, self.low, self.high, self.n_per = net, low, high, n_per
        # None: modelPN.default_precision — the exact split wherever its kernels apply (what bench.py measures), else fp32;
        # "f16": opt-in fp16-operand encoder (not parity-exact)
        self.precision = default_precision(low, high) if precision is None else precision
        self.cache_service_embedding = True   # False: re-evaluate the GCN branch in every pass (round-1 behaviour)
        self._side_streams = {}
        warn_partitioned_device(next(low.parameters()).device, self.precision)

    @torch.no_grad()
    def service_embedding(self, services):
        """The GCN (service) branch of Net.forward (modelML.py:145-156,164): a function of the weights and the service
        table ONLY, so it is evaluated once per (weights, table) and kept on the table ("compute
        the service embedding once per model and cache it") instead of once per batch.  Loading / moving the weights
        gives a new prepared-weights object and so invalidates the entry."""
        prep = self.net.prepared(services.x_service.device)
        c = services.emb_cache
        if c is None or c[0] is not prep:
            c = services.emb_cache = (prep, self.net.service_embedding(services.x_service, services.csr))
        return c[1]

    @torch.no_grad()
    def scores(self, services, batch):
        """TrainML.test's forward (trainML.py:56-58)."""
        return self.net.scores(batch.x, batch.wf_csr, batch.seg_ptr, services.x_service, services.csr,
                               service_emb=self.service_embedding(services) if self.cache_service_embedding else None,
                               max_nodes=batch.max_nodes, dense_precision="split" if self.precision == "split" else "f32")

    @torch.no_grad()
    def candidates(self, services, batch, scores):
        """sort + loadDataPN + SCDataset, fused (trainML.py:62; loadData.py:101-149; trainPNHigh.py:23-31)."""
        return torch.ops.gnnpn.segment_topk_feasible(scores, services.cat_ptr, services.qos, batch.local_bounds,
                                                     batch.present, batch.global_bounds, self.n_per)

    @torch.no_grad()
    def score_select_operands(self, services, batch):
        """(packed service embedding, plan_host, plan) of the one-launch score product + candidate reduction
        (torch.ops.gnnpn.score_select, csrc/score_select.hip), or None where the two launches stay: GNNPN_UNFUSED_FRONT=1, the
        service embedding not cached, or a shape the kernel is not built for (score_plan.applies: hidden 128, n_per <= 16, mean
        category >= 16 services, largest <= 256 — the 1000- and 2000-task shapes with 5 or 10 services per category keep
        select.hip's 8-lane form).  The packed embedding follows the service embedding (one per (weights, table)); the chunk plan
        depends on the table only and is kept per chunk count — about one workgroup per CU for this batch's tiles of 16 problems."""
        if score_plan.unfused_front() or not self.cache_service_embedding:
            return None
        c = services.score_cache
        if c is None:
            c = services.score_cache = score_plan.OperandCache(services.cat_ptr.cpu().numpy(), services.qos.device)
        if not c.applies(self.net.nodeLin.weight.shape[0], self.n_per):
            return None
        n_cu = torch.cuda.get_device_properties(c.device).multi_processor_count
        planned = c.plan(score_plan.chunk_count(c.n_categories, batch.n_problems, n_cu))
        if planned is None:
            return None
        plan, plan_host, plan_dev = planned
        return c.packed(self.service_embedding(services), plan), plan_host, plan_dev

    @torch.no_grad()
    def front(self, services, batch):
        """scores [B,S], pn_inputs rows [B, T*n_per, 8], candidate_ids: ``scores`` then ``candidates``, or the one launch that
        computes the same three (``score_select_operands``) behind the request branch."""
        fused = self.score_select_operands(services, batch)
        if fused is None:
            scores = self.scores(services, batch)
            return (scores, *self.candidates(services, batch, scores))
        xr = self.net.request_embedding(batch.x, batch.wf_csr, batch.seg_ptr, batch.max_nodes,
                                        "split" if self.precision == "split" else "f32")
        return torch.ops.gnnpn.score_select(xr, *fused, services.qos, batch.local_bounds, batch.present, batch.global_bounds, self.n_per)

    @torch.no_grad()
    def run(self, services, batch, decode_impl=0, lds_kb=0, ws=None, paired_start=False, write_through=False):
        """One pass.  decode_impl / lds_kb / paired_start / ws: launch options of the recurrent kernels (modelPN.two_level_greedy;
        paired_start: the caller starts these launches together with a partner's — half-batches do by construction).
        ``ws`` = a PAIR of workspaces: the recurrent part runs as two half-batches side by side, the second on a side
        stream (fork / join, capturable) — the problems are independent, and two cooperative launches of one workgroup
        per CU each share every CU for their whole length (encoder beside encoder, decoder beside decoder), which two
        whole batches in flight on two slots do only where their timelines happen to line up."""
        scores, rows, ids = self.front(services, batch)
        if isinstance(ws, (tuple, list)):
            B = rows.shape[0]
            half = half_batch_split(B)
            if len(ws) != 2 or not half:
                raise ops.GnnpnError(f"ML2PNPipeline.run: two half-batches need 2 workspaces and more than 16 problems (got {len(ws)}, {B})")
            cur = torch.cuda.current_stream(rows.device)
            side = self._side_streams.get(rows.device)
            if side is None:
                side = self._side_streams[rows.device] = torch.cuda.Stream(rows.device)
            # everything both halves share is produced on the CURRENT stream before the fork: the packed / folded weights
            # (pack kernels and host-to-device copies of a first call) and the lazily allocated workspaces would otherwise be
            # issued on the side stream by the half that runs first in Python, with nothing ordering the other half's
            # reads behind them
            for net in (self.low, self.high):
                net.actor.packed()
                net.actor.check_precision(self.precision)
            n_cat = rows.shape[1] // self.n_per
            for w in ws:
                w.encode()
                w.decode(max(half, B - half), n_cat, self.n_per)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                out_b = two_level_greedy(self.low, self.high, rows[half:], precision=self.precision, decode_impl=decode_impl,
                                         lds_kb=lds_kb, ws=ws[1], paired_start=True, write_through=write_through)
            out_a = two_level_greedy(self.low, self.high, rows[:half], precision=self.precision, decode_impl=decode_impl,
                                     lds_kb=lds_kb, ws=ws[0], paired_start=True, write_through=write_through)
            cur.wait_stream(side)
            for v in out_b.values():
                v.record_stream(cur)
            out = {k: torch.cat([out_a[k], out_b[k]]) for k in out_a}
        else:
            out = two_level_greedy(self.low, self.high, rows, precision=self.precision, decode_impl=decode_impl,
                                   lds_kb=lds_kb, ws=ws, paired_start=paired_start, write_through=write_through)
        out.update(scores=scores, pn_inputs=rows, candidate_ids=ids)
        return out

    @torch.no_grad()
    def best_of(self, services, batch, samples, seed=None, decode_impl=0, lds_kb=0, ws=None, write_through=False, return_all=False):
        """One pass with best-of-``samples`` decoding of the High level (modelPN.two_level_best_of): scores -> candidates ->
        the greedy pass plus samples-1 sampled High replicas, the one with the smallest R per problem.  Returns run's keys (the
        winners) plus sample_index, R_all and idx_all.  seed None: fresh OS entropy.  A separate call: run / capture are
        unchanged; not capturable (it checks the cooperative launches' status before it returns).  ``return_all``: also actions_all
        [B, samples, T, 8|9], every replica's rows (replica 0 the greedy ones): the starts of ``descend_starts``."""
        scores, rows, ids = self.front(services, batch)
        out = two_level_best_of(self.low, self.high, rows, samples, seed=seed, precision=self.precision, decode_impl=decode_impl,
                                lds_kb=lds_kb, write_through=write_through, ws=ws, return_all=return_all)
        out.update(scores=scores, pn_inputs=rows, candidate_ids=ids)
        return out

    def refine(self, services, batch, out, popSize, MAX_Iter, reduct=0, seeds=None, min_cost=None, patches=()):
        """The third stage, ES-WOA refinement of ``out["actions"]`` on the device: module-level ``refine`` (it needs no
        network).  An extra call: ``run`` / ``capture`` are unchanged."""
        return refine(services, batch, out, popSize, MAX_Iter, reduct=reduct, seeds=seeds, min_cost=min_cost, patches=patches)

    def descend(self, services, batch, out, max_sweeps=16, reduct=0, min_cost=None, patches=()):
        """One-swap descent of ``out["actions"]`` on the device: module-level ``descend`` (it needs no network).  An extra call:
        ``run`` / ``capture`` are unchanged."""
        return descend(services, batch, out, max_sweeps=max_sweeps, reduct=reduct, min_cost=min_cost, patches=patches)

    def descend_starts(self, services, batch, starts, max_sweeps=16, reduct=0, min_cost=None, patches=()):
        """Multi-start descent from ``best_of(..., return_all=True)``'s replicas (or any [B, N, T, 8|9] rows): module-level
        ``descend_starts`` (it needs no network).  An extra call: ``run`` / ``capture`` are unchanged."""
        return descend_starts(services, batch, starts, max_sweeps=max_sweeps, reduct=reduct, min_cost=min_cost, patches=patches)

    def descend_pairs(self, services, batch, out, max_sweeps=16, max_rounds=4, reduct=0, min_cost=None, patches=()):
        """Pair-swap descent of ``out["actions"]`` on the device: module-level ``descend_pairs`` (it needs no network).  An extra
        call: ``run`` / ``capture`` are unchanged."""
        return descend_pairs(services, batch, out, max_sweeps=max_sweeps, max_rounds=max_rounds, reduct=reduct, min_cost=min_cost,
                             patches=patches)

    def descend_pairs_windowed(self, services, batch, out, max_sweeps=16, max_rounds=4, max_span=0, reduct=0, min_cost=None, patches=()):
        """Pair-swap descent at any slot count, over slots at most ``max_span`` apart (0: all): module-level
        ``descend_pairs_windowed`` (it needs no network).  An extra call: ``run`` / ``capture`` are unchanged."""
        return descend_pairs_windowed(services, batch, out, max_sweeps=max_sweeps, max_rounds=max_rounds, max_span=max_span, reduct=reduct,
                                      min_cost=min_cost, patches=patches)

    def descend_pairs_shortlist(self, services, batch, out, max_sweeps=16, max_rounds=4, max_span=0, max_rank=0, reduct=0, min_cost=None,
                                patches=()):
        """Pair-swap descent of ``out["actions"]`` over shortlists of each slot's best candidates: module-level
        ``descend_pairs_shortlist`` (it needs no network).  An extra call: ``run`` / ``capture`` are unchanged."""
        return descend_pairs_shortlist(services, batch, out, max_sweeps=max_sweeps, max_rounds=max_rounds, max_span=max_span,
                                       max_rank=max_rank, reduct=reduct, min_cost=min_cost, patches=patches)

    def descend_starts_pairs_shortlist(self, services, batch, starts, max_sweeps=16, pair_rounds=4, pair_span=0, pair_rank=0, reduct=0,
                                       min_cost=None, patches=()):
        """Multi-start pair-swap descent at any slot count, over a span and shortlists: module-level ``descend_starts_pairs_shortlist``
        (it needs no network).  An extra call."""
        return descend_starts_pairs_shortlist(services, batch, starts, max_sweeps=max_sweeps, pair_rounds=pair_rounds, pair_span=pair_span,
                                              pair_rank=pair_rank, reduct=reduct, min_cost=min_cost, patches=patches)

    def descend_starts_pairs(self, services, batch, starts, max_sweeps=16, pair_rounds=4, reduct=0, min_cost=None, patches=()):
        """Multi-start pair-swap descent: module-level ``descend_starts_pairs`` (it needs no network).  An extra call."""
        return descend_starts_pairs(services, batch, starts, max_sweeps=max_sweeps, pair_rounds=pair_rounds, reduct=reduct,
                                    min_cost=min_cost, patches=patches)

    def descend_tabu(self, services, batch, out, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, reduct=0, min_cost=None, patches=()):
        """Tabu walk of ``out["actions"]`` from its one-swap optimum: module-level ``descend_tabu`` (it needs no network).  An extra
        call: ``run`` / ``capture`` are unchanged."""
        return descend_tabu(services, batch, out, max_sweeps=max_sweeps, max_steps=max_steps, tenure=tenure, reduct=reduct,
                            min_cost=min_cost, patches=patches)

    def descend_tabu_pairs(self, services, batch, out, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, max_rank=ops.DEFAULT_PAIR_RANK,
                           max_span=0, reduct=0, min_cost=None, patches=()):
        """Tabu walk over pair moves of ``out["actions"]``: module-level ``descend_tabu_pairs`` (it needs no network).  An extra call."""
        return descend_tabu_pairs(services, batch, out, max_sweeps=max_sweeps, max_steps=max_steps, tenure=tenure, max_rank=max_rank,
                                  max_span=max_span, reduct=reduct, min_cost=min_cost, patches=patches)

    def descend_starts_tabu_pairs(self, services, batch, starts, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE,
                                  max_rank=ops.DEFAULT_PAIR_RANK, max_span=0, reduct=0, min_cost=None, patches=()):
        """Multi-start tabu walk over pair moves: module-level ``descend_starts_tabu_pairs`` (it needs no network).  An extra call."""
        return descend_starts_tabu_pairs(services, batch, starts, max_sweeps=max_sweeps, max_steps=max_steps, tenure=tenure, max_rank=max_rank,
                                         max_span=max_span, reduct=reduct, min_cost=min_cost, patches=patches)

    def descend_starts_tabu(self, services, batch, starts, max_sweeps=16, max_steps=32, tenure=ops.DEFAULT_TENURE, reduct=0, min_cost=None,
                            patches=()):
        """Multi-start tabu walk: module-level ``descend_starts_tabu`` (it needs no network).  An extra call."""
        return descend_starts_tabu(services, batch, starts, max_sweeps=max_sweeps, max_steps=max_steps, tenure=tenure, reduct=reduct,
                                   min_cost=min_cost, patches=patches)

    def capture(self, services, batch, warmup=2, decode_impl=0, lds_kb=0, ws=None, paired_start=False, pool=None, write_through=False):
        """Record one whole pass over (services, batch) into a HIP graph and return a callable that
        replays it on the CURRENT stream (one launch per step instead of ~25).  The returned dict's
        tensors are the graph's static outputs: they are overwritten by every replay.  ``ws`` is the
        private ``ops.Workspaces`` of this graph (default: a new one), so that graphs may be in flight
        at the same time on different streams (independent batches pipelined); it is frozen — the graph
        holds its addresses — and lives as long as the returned callable.  ``pool``: a graph memory pool to capture
        into (torch.cuda.graph's argument; NOT for graphs whose outputs must survive each other's replays)."""
        ws = ops.new_workspaces(batch.x.device) if ws is None else ws
        all_ws = list(ws) if isinstance(ws, (tuple, list)) else [ws]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(warmup):          # allocate workspaces / pack weights outside the capture
                self.run(services, batch, decode_impl, lds_kb, ws, paired_start, write_through)
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # thread_local: only THIS thread's calls are policed during the capture.  In the default ("global") mode an event query
        # made by another thread while the capture is open is an error that invalidates it — and the watchdog thread of
        # torch.distributed's RCCL process group queries the events of its collectives whenever one is outstanding: a runner
        # captured while collectives are in flight (bench.py's degraded form at N > 1 is built mid-run) died that way in one
        # of this round's GPU runs (ProcessGroupNCCL watchdog: HIP error from hipEventQuery, the process aborted)
        with torch.cuda.graph(graph, pool=pool, capture_error_mode="thread_local"):
            out = self.run(services, batch, decode_impl, lds_kb, ws, paired_start, write_through)
        for w in all_ws:
            w.frozen = True
        booked_replay = ops.graph_replay(graph, all_ws)      # graph.replay() + the host's count of the cooperative launches it makes

        def replay():
            booked_replay()
            return out
        replay.graph, replay.outputs, replay.workspaces = graph, out, ws
        return replay

    @torch.no_grad()
    def rankings(self, services, batch):
        """The artefact TrainML.test writes (trainML.py:62-68,148-149): full ranking per problem."""
        return torch.ops.gnnpn.rank_rows(self.scores(services, batch))

    @torch.no_grad()
    def test(self, services, batch, labels):
        """TrainML.test (trainML.py:49-72): (idxList = full ranking per problem, [P@1, P@5]).
        ``labels`` [B,S] 0/1 (float32 device tensor).  Rankings stay on the device (int32 [B,S])."""
        ranking = self.rankings(services, batch)
        pk = torch.ops.gnnpn.precision_at_k(ranking, labels.float().contiguous(), [1, 5])
        return ranking, [float(v) for v in pk.mean(0).tolist()]


# device index -> weak reference to the PipelinedRunner whose replays were enqueued last on that device (PipelinedRunner._take_turn)
_last_runner_on_device = {}


def _has_collective_stream():
    """True in a rank of an RCCL ("nccl") process group: its collectives run on a stream of the process group's own."""
    import torch.distributed as td
    if not (td.is_available() and td.is_initialized()):
        return False
    try:
        return "nccl" in str(td.get_backend()).lower()
    except Exception:       # a backend object without a name: assume it brings a stream
        return True


def _hw_queues(env=None):
    """The number of in-order hardware queues the HIP runtime deals this process's streams onto (unset or empty: its default, 4)."""
    return int((os.environ if env is None else env).get("GPU_MAX_HW_QUEUES", "4") or 4)


def _separate_priority(n_streams, collective_stream, env=None):
    """The priority PipelinedRunner's slot streams get where nobody names one: -1, a priority of their own, for free-running slots
    in a rank of an RCCL process group that has fewer than 8 hardware queues, else 0 (runner_plan says why)."""
    return -1 if n_streams > 1 and collective_stream and _hw_queues(env) < 8 else 0


def _pinned_host(arena):
    """Whether a packed batch's arena is pinned host memory (``PipelinedRunner.pack_host``): one asynchronous host-to-device copy."""
    return arena.device.type == "cpu" and arena.is_pinned()


@dataclass(frozen=True)
class RunnerPlan:
    """The mode of a PipelinedRunner: every decision ``runner_plan`` makes, under the names of the runner's attributes."""
    n_slots: int                 # static input / output sets = the reuse distance of submit()'s outputs
    halves: bool                 # ONE batch in flight, its recurrent part as two half-batches side by side
    n_streams: int               # steps in flight (1 or 2)
    n_workspaces: int
    stream_priority: int
    priority_chosen: bool        # neither the argument nor GNNPN_PIPE_STREAM_PRIORITY named the priority: runner_plan chose it
    decode_impl: int
    lds_kb: tuple                # LDS footprint of the cooperative launches, per slot
    front_lds_kb: int            # ... and of the ordinary LDS-using kernels in front of them
    lockstep: bool               # the two slots' replays start in pairs
    common_start_us: float       # > 0: the first replays of a burst are held behind a gate, at most this long
    write_through: bool


def runner_plan(n_problems, slots, precision, seq_len, *, halves=None, stream_priority=None, write_through=None, env=os.environ,
                collective_stream=False):
    """The mode of a PipelinedRunner over batches of ``n_problems`` with ``slots`` slots, for a pipeline of ``precision`` whose
    recurrences run ``seq_len`` steps per problem (T * K): a pure function of its arguments and ``env``.  ``halves``,
    ``stream_priority``, ``write_through``: the constructor's arguments (None: decided here); ``collective_stream``: this process
    is a rank of an RCCL process group (``_has_collective_stream``).  The environment variables it reads, each with its default:

        GNNPN_PIPE_HALVES            "0": never pair half-batches (default: pair them from 512 problems on, with more than one slot)
        GNNPN_PIPE_STREAM_PRIORITY   the slot streams' priority (default: -1 for free-running slots beside a collective stream with
                                     fewer than 8 hardware queues — ``_hw_queues`` —, else 0); the argument wins
        GNNPN_PIPE_DECODE_IMPL       the decoder build (default: 4 where two cooperative launches share every CU, else 0 = auto)
        GNNPN_SLOT_LDS_KB            the cooperative launches' LDS footprint in KB, one entry per slot, comma-separated (default: 78
                                     each with the exact split where launches share CUs, else 0 = the kernel's own)
        GNNPN_PIPE_FRONT_LDS_KB      the footprint of the ordinary kernels in front of them (default: the same 78 for two
                                     free-running slots, else 0)
        GNNPN_PIPE_LOCKSTEP          "1" / "0": two slots start their replays in pairs (default: from 2000 recurrent steps on)
        GNNPN_PIPE_COMMON_START_US   the longest hold of a burst's first replays behind the common-start gate (default:
                                     COMMON_START_US = 0, no gate); two free-running slots without lockstep only

    (GNNPN_PIPE_WRITE_THROUGH and GNNPN_HOST_COPY_INLINE are read once, when this module is imported: DEFAULT_WRITE_THROUGH and
    HOST_COPY_ON_ITS_OWN_STREAM above.)  A GNNPN_SLOT_LDS_KB list shorter than the slots raises GnnpnError."""
    # Batches of 512 problems and more: ONE batch in flight, its recurrent part as two half-batches side by side
    # (ML2PNPipeline.run with a pair of workspaces).  A cooperative launch has one workgroup per CU and two of them
    # fill a CU's registers, so nothing else runs beside a co-resident pair; with two WHOLE batches in flight on two
    # slots the pairing is left to chance — one slot's front half waits for the other's 25 ms encoder, encoders meet
    # decoders — and the 1000-task shape ran 28.3 ms per batch where its recurrent kernels, always paired, need 21.1
    # (tools/bench_slot_parts.py).  Below 512 problems a half-batch launch no longer fills the chip: two slots.
    halves = bool(halves) if halves is not None else (n_problems >= 512 and int(slots) > 1 and env.get("GNNPN_PIPE_HALVES", "1") != "0")
    # ``n_slots`` = the number of static input / output sets = the reuse distance of submit()'s outputs, in EVERY mode
    # (the half-batch mode used to collapse to one slot, and a caller following the documented rule read
    # outputs the next replay was already overwriting).  ``n_streams`` = steps in flight: the half-batch mode keeps ONE
    # step in flight, so its slots' graphs replay one after the other on one stream.
    n_slots = max(1, int(slots))
    # ... and never more than TWO: a CU holds two cooperative workgroups, so two replays in flight are what the chip has room for —
    # a third free-running stream put three launches in front of those two slots and ended in half-staffed launches and
    # bounded-wait time-outs (round 6, tools/probes/dbg_three_slots.py: slots=3 ran 24 k problems/s with status 0x13).  More slots
    # than two are more static input / output sets (a longer reuse distance), dealt onto the two streams in turn.
    n_streams = 1 if halves else min(n_slots, 2)
    # Stream priority of the slots: HIP deals a process's streams onto a few in-order hardware queues (_hw_queues,
    # default 4) round robin, PER PRIORITY.  In a rank of an RCCL process group the collective's stream waits for one slot's
    # step; when that wait shares a hardware queue with the other slot's stream it sits in front of that slot's launches
    # (forced world-1 all-gather at the QWS shape: 449 k problems/s against 480 k without a process group).  Slot streams of a
    # priority of their own never share a queue with the process group's (normal-priority) stream: 470 k, the same as 8
    # hardware queues give (467 k) but without an environment variable that has to be set before the runtime starts — and
    # the two do NOT add up (8 queues AND high priority: 367-378 k).  Without a process group high priority costs 0.35 %
    # (477.8-478.2 k against 479.5-479.7 k), so it is used only where a collective stream exists.  profiles/LOG_r06.md §9.
    # (a process started with 8 or more hardware queues has the separation already — and must not get both)
    # Only for free-running slots on streams of their own: the half-batch mode keeps ONE step in flight on one stream (nothing of
    # another slot for the collective's wait to sit in front of), and there high priority COSTS — Normal shape, forced RCCL:
    # 199 k problems/s against 234-238 k at normal priority (238 k without a process group); 1000-task shape 22.8 k against 23.8 k
    # (tools/r06/dist_priority_shapes.sh)
    named = env.get("GNNPN_PIPE_STREAM_PRIORITY")
    priority_chosen = stream_priority is None and named is None
    if stream_priority is None:
        stream_priority = int(named) if named is not None else _separate_priority(n_streams, collective_stream, env)
    # decoder form beside another slot's kernels: the 8-member build sized for two workgroups per CU (decode_impl 4).  Measured at QWS B=256 against the 16-member form (3):
    # 228 k vs 221 k problems/s in fp32, 353 k vs 316 k with the split precision.
    shared = 4
    paired = n_streams > 1 or halves    # two cooperative launches share every CU
    decode_impl = int(env.get("GNNPN_PIPE_DECODE_IMPL", shared if paired else 0))
    # Placement: the cooperative kernels claim one CU per workgroup at run time (csrc/coop_common.h, coop_place), so
    # the two slots' launches share every CU one workgroup each whatever the dispatcher does; the LDS-footprint
    # padding round 1 steered the dispatcher with (100 / 56 KB) is no longer needed and stays as an option only.
    # Exact-split precision: the recurrent kernels hold the third weight piece in LDS (60 KB encoder, 69 KB decoder).  Two
    # such workgroups fit a CU's 160 KB, but LDS is allocated in CONTIGUOUS ranges: with unequal footprints a freed 60 KB
    # hole does not take the next 69 KB workgroup while the neighbour's range sits in the middle, the launch stays
    # under-staffed, and two launches can starve each other until the bounded spins give up (seen: bench.py, precision
    # split, two slots: members missing at the first sweep, 20 of 32 seats of an XCD staffed after 0.3 s).  Every
    # cooperative launch of a multi-slot runner is therefore padded to ONE footprint, 78 KB: any freed range fits any
    # waiting workgroup.  (f32: 19 / 27 KB — nothing to equalise.)
    named = env.get("GNNPN_SLOT_LDS_KB")
    equal = 78 if (precision == "split" and paired) else 0
    lds_kb = tuple(int(v) for v in named.split(",")) if named else (equal,) * n_slots
    if len(lds_kb) < n_slots:            # (used to end in an IndexError in the middle of the captures)
        raise ops.GnnpnError(f"GNNPN_SLOT_LDS_KB={named!r} has {len(lds_kb)} entries for {n_slots} slots: one footprint per slot")
    # ... and so are the ORDINARY kernels of a step that use LDS in front of the encoder (the one-launch GIN branch, the score
    # product: ops.lds_footprint / gnnpn_lds_footprint_kb).  A cooperative workgroup that lands above such a kernel's few KB
    # keeps its 78 KB in the middle of the CU when the small kernel has gone, and the OTHER slot's encoder workgroup for that
    # CU finds no contiguous 78 KB until this encoder has finished: the two free-running slots slipped apart by 0.5 ms in
    # every 20-step round (round 4 held the slots of a burst behind a common-start gate against it: 455 k problems/s with 4-8
    # slow rounds of 89; with the front half at the same footprint 460 k and no slow round in 270, gate off —
    # profiles/r05_slip_front_lds.jsonl).  Two free-running slots only: the half-batch mode runs its front half alone.
    named = env.get("GNNPN_PIPE_FRONT_LDS_KB")
    front_lds_kb = int(named) if named is not None else (equal if (n_streams == 2 and not halves) else 0)
    # Two slots, long recurrent kernels: start the two replays of a pair TOGETHER (a submission joins the leader that is
    # still waiting for a partner, else it leads).  Free-running slots drift apart by the difference of their step
    # times, and a cooperative launch that starts under the OTHER slot's front half finds every CU's LDS occupied by
    # short-lived neighbours: its workgroups land above them (coop_place gives such seats back, up to a few hundred times
    # per launch), seats are taken off their canonical CUs, and from there on both slots' launches run at the speed of
    # one — the 2000-task shape alternated between 41 and 62 ms per step (spread 37-48 % over rounds; tools/slot_overlap.py).
    # Started together, the two front halves run side by side and are gone when the encoders arrive.  The wait costs the
    # tail by which the two replays differ (2 % at that shape); short steps (QWS, Normal) keep running free.
    named = env.get("GNNPN_PIPE_LOCKSTEP")
    long_steps = int(seq_len) >= 2000          # recurrent steps per problem (T * K)
    lockstep = n_slots == 2 and n_streams == 2 and (named == "1" or (named is None and long_steps))
    # Common start of a burst (two free-running slots only).  Two slots that begin a burst a host enqueue apart (~0.1 ms:
    # the second replay is not in its queue yet when the first starts) run in step for a few steps and then slip apart ONCE
    # — one slot's step takes 1.7 instead of 1.2 ms at the QWS shape — which costs a 20-step burst 0.5 ms (4 %); slots
    # released TOGETHER stay in step (tools/probes/stagger_probe.py: 11.50 against 12.01 ms per 20 steps, the hold included;
    # 30 and 60 us are too short, 90 and more work).  So the first replay after the runner has been idle is held behind a
    # gate on another stream, and so is the other slot's first one; later replays are not.  The gate (gnnpn_gate_wait: one
    # wavefront polling a word in pinned host memory) is opened by the HOST the moment the second replay is in its queue —
    # or by synchronize / poll, or after COMMON_START_US at the latest (a burst of one replay that is waited for some other way).
    # "Idle" = since the last synchronize() / poll() of this runner: a caller that works in bursts waits for them that way.
    common_start_us = float(env.get("GNNPN_PIPE_COMMON_START_US", COMMON_START_US)) \
        if (n_slots == 2 and n_streams == 2 and not lockstep) else 0.0
    # write_through: the placement-independent hand-off form (agent-scope write-through granule stores) in every cooperative
    # launch of this runner — the degraded mode bench.py falls back to when a launch reported a failed hand-off
    write_through = DEFAULT_WRITE_THROUGH if write_through is None else bool(write_through)
    return RunnerPlan(n_slots=n_slots, halves=halves, n_streams=n_streams, n_workspaces=2 if halves else n_slots,
                      stream_priority=int(stream_priority), priority_chosen=priority_chosen, decode_impl=decode_impl, lds_kb=lds_kb,
                      front_lds_kb=front_lds_kb, lockstep=bool(lockstep), common_start_us=common_start_us, write_through=write_through)


class PipelinedRunner:
    """Throughput mode: ``slots`` independent batches in flight on ``slots`` HIP streams — or, for batches of 512 problems
    and more, ONE batch in flight whose recurrent part runs as two half-batches side by side (``halves``: the ``slots``
    static input / output sets then take turns on one stream); two slots with recurrences of 2000 steps and more start
    their replays in pairs (``lockstep``).  In every mode ``n_slots`` is the reuse distance of ``submit``'s outputs.
    See runner_plan.

    The recurrent kernels are step-latency-bound and leave most of the machine idle, so consecutive
    (independent) batches are overlapped: every slot owns one captured HIP graph of the whole pass, its
    own static input/output tensors and its own cooperative-kernel hand-off workspaces; batch i runs on
    slot i % slots.  With two slots the 16-member decoder form is selected (256 registers: it shares
    every SIMD with a wave of the other slot's encoder).  All batches must have the shapes of
    ``example_batch`` (graphs are shape-static); ``submit`` copies a new batch into the slot's static
    tensors on the slot's stream (``batch=None`` re-runs the resident one, as bench.py does).
    """

    def __init__(self, pipe, services, example_batch, slots=2, halves=None, write_through=None, auto_degrade=True,
                 stream_priority=None):
        plan = self.plan = runner_plan(example_batch.n_problems, slots, getattr(pipe, "precision", "f32"),
                                       int(getattr(pipe.low.actor, "seq_len", 0)), halves=halves, stream_priority=stream_priority,
                                       write_through=write_through, collective_stream=_has_collective_stream())
        self.pipe, self.services = pipe, services
        self.halves, self.n_slots, self.n_streams, self.stream_priority = plan.halves, plan.n_slots, plan.n_streams, plan.stream_priority
        self.decode_impl, self.lds_kb, self.front_lds_kb = plan.decode_impl, list(plan.lds_kb), plan.front_lds_kb
        self.lockstep, self.common_start_us, self.write_through = plan.lockstep, plan.common_start_us, plan.write_through
        self.streams = [torch.cuda.Stream(priority=self.stream_priority) for _ in range(self.n_streams)]
        self.count = 0
        self._copy_streams = [torch.cuda.Stream() for _ in range(self.n_slots)]   # host-to-device transfers of pinned arenas (submit)
        self._gate_flag = torch.zeros(1, dtype=torch.int32).pin_memory() if self.common_start_us > 0 else None   # the word the gate polls
        self._gate_seq = 0                       # value that opens the current gate (one more per burst)
        # (the gate's spin runs on slot 0's transfer stream, idle whenever the batches are resident: one more stream of its own
        # changed which streams share a hardware queue and cost the pinned-host path 1.7 %)
        self._gate_stream = self._copy_streams[0] if self.common_start_us > 0 else None
        self._idle()
        # gnnpn_launch_opts_t.paired_start: half-batches (set inside ML2PNPipeline.run) and slots started in pairs begin together
        self.batches = [self._clone(example_batch) for _ in range(self.n_slots)]   # never alias caller tensors
        self.workspaces = [ops.new_workspaces(example_batch.x.device) for _ in range(plan.n_workspaces)]
        # (every graph keeps its OWN memory pool, also the half-batch mode's two that never run together: in a shared pool
        # the second capture places its outputs where the first keeps intermediates, and the first graph's next replay
        # writes over them — measured: garbage in a slot's outputs one submission later)
        # auto_degrade: the first poll / synchronize that finds a failed launch (any status code, the shortfall of finished
        # workgroup-tiles included) re-captures every slot with the write-through hand-off; ``degraded`` keeps the status that
        # caused it.  The batches since the previous poll are invalid either way and the caller submits them again.
        self.auto_degrade, self.degraded = bool(auto_degrade), None
        self._capture_graphs()

    def _idle(self):
        """The start coordination (pairs of ``lockstep``, the deferred leader, the common-start gate) with nothing in flight and
        nobody waiting: a new runner's, and that of one whose graphs are captured anew (``_degrade``, behind ``_wait``)."""
        self._open_leader, self._last_done = None, [None] * max(2, self.n_slots)
        self._slot_done = [None] * self.n_slots
        self._deferred = None                    # (slot, after): a leader whose replay waits for its partner's submission (submit)
        self._gate = None                        # [event, slots still to be held behind it]
        self._drained = True                     # nothing in flight: set by synchronize / poll, cleared by the next replay

    def _capture_graphs(self):
        with ops.lds_footprint(self.front_lds_kb):            # captured launches keep the footprint (a per-launch attribute)
            self.graphs = [self.pipe.capture(self.services, self.batches[s], decode_impl=self.decode_impl, lds_kb=self.lds_kb[s],
                                             ws=tuple(self.workspaces) if self.halves else self.workspaces[s], paired_start=self.lockstep,
                                             write_through=self.write_through)
                           for s in range(self.n_slots)]

    def _degrade(self, word):
        """A launch of this runner failed (status ``word``): from now on every cooperative launch uses the placement-independent
        write-through hand-off (new graphs over the same static inputs and workspaces; the old ones are dropped)."""
        if not self.auto_degrade or self.write_through:
            return
        import warnings
        warnings.warn(f"gnnpn: PipelinedRunner: cooperative launches reported status {word:#x}; switching this runner to the "
                      f"write-through hand-off (the batches since the last poll / synchronize must be submitted again)", RuntimeWarning)
        self.write_through, self.degraded = True, word
        self._idle()
        self._capture_graphs()

    @staticmethod
    def _fields(b):
        return (b.x, b.wf_csr.rowptr, b.wf_csr.col, b.seg_ptr, b.local_bounds, b.present, b.global_bounds)

    @classmethod
    def _clone(cls, b, host=False):
        """A copy of the batch whose seven tensors are views into ONE allocation (``_arena``, 256-byte aligned pieces): a
        batch that was packed the same way (``pack``) moves into a slot's static inputs with one copy instead of seven —
        at a 0.55 ms step seven 5 us copy kernels in front of every replay are 3 % of the slot's cycle.  ``host``: the
        arena in PINNED host memory (``pack_host``): the same single copy, now host-to-device."""
        fields = cls._fields(b)
        offs, total = [], 0
        for t in fields:
            offs.append(total)
            total += (t.numel() * t.element_size() + 255) // 256 * 256
        arena = (torch.empty(max(total, 256), dtype=torch.uint8, pin_memory=True) if host else
                 torch.empty(max(total, 256), dtype=torch.uint8, device=b.x.device))
        views = []
        for t, o in zip(fields, offs):
            v = arena[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
            v.copy_(t)
            views.append(v)
        x, rowptr, col, seg, lb, pr, gb = views
        out = DeviceBatch(x, graph.CSR(rowptr, col, None, b.wf_csr.n), seg, lb, pr, gb, b.max_nodes)
        out._arena, out._layout = arena, tuple((tuple(t.shape), t.dtype) for t in fields)
        return out

    def pack(self, batch):
        """The batch in the slots' own memory layout: ``submit`` moves such a batch with a single device-to-device copy."""
        return self._clone(batch)

    def pack_host(self, batch):
        """The batch (host or device tensors) in the slots' layout in ONE pinned host allocation: ``submit`` moves it into a
        slot's static inputs with a single asynchronous host-to-device copy on the slot's stream — the reference's per-batch
        ``inputs.cuda()`` (src/models/trainPNHigh.py:134-136) as one copy instead of seven.  The caller must not rewrite the
        arena before that copy has run (record an event on ``stream(slot)``)."""
        return self._clone(batch, host=True)

    def submit(self, batch=None, after=None):
        """Enqueue one batch; returns (outputs dict, slot).  The outputs are the slot's static tensors:
        consume them (or record an event on ``stream(slot)``) before the slot comes round again, ``n_slots`` submits
        later — in every mode (half-batch mode included: there the slots alternate on one stream).
        ``after(outputs, slot)``: called with the slot's stream current, right behind the enqueued replay — the place for the
        device-to-host copies of the results.  It matters for slots that start in PAIRS (``lockstep``) when the batch comes from a
        pinned host arena: the leader's replay is then enqueued together with its partner's, once BOTH transfers are on their way
        (each replay waits for both), so that the pair still starts together; ``after`` of the leader runs at that moment.
        Touching ``stream(slot)``, ``poll`` or ``synchronize`` enqueues a waiting leader at once (alone)."""
        s = self.count % self.n_slots
        if self.count == 0 and self.plan.priority_chosen and self.stream_priority == 0 and \
                _separate_priority(self.n_streams, _has_collective_stream()) != 0:
            import warnings                                # the process group came AFTER this runner: its streams were created at normal priority
            warnings.warn("PipelinedRunner was created before the RCCL process group: its slots' streams share hardware queues with the "
                          "collective's stream (about 6 % slower with one all-gather per 8 steps at the QWS shape); create the runner after "
                          "init_process_group, or pass stream_priority=-1", RuntimeWarning, stacklevel=2)
        self._take_turn()
        self.count += 1
        if self._deferred is not None and self._deferred[0] == s:
            self._flush_deferred()
        staged = batch is not None and self._load(s, batch)
        if self.lockstep and staged:
            # Pairs and transfers: two transfers of a pair run one after the other on the copy engine (0.7 ms each at the 2000-task
            # shape), so a leader that starts behind ITS transfer is that far ahead of its partner, its encoder arrives while the
            # partner's front half still holds CUs, and the common start the pairing exists for is gone (PCIe-inclusive rate 0.57
            # of the resident one).  The leader's replay therefore waits here, on the host side, for its partner's submission.
            if self._deferred is None:
                self._deferred = (s, after)
                return self.graphs[s].outputs, s
            lead, after_lead = self._deferred
            self._deferred = None
            return self._replay_pair(lead, after_lead, s, after), s
        self._flush_deferred()
        if batch is not None and self.common_start_us > 0:
            arena = getattr(batch, "_arena", None)
            if (arena if arena is not None else batch.x).device.type == "cpu":
                self._drained = False                # batches from host memory: no common start (their transfers share the copy
                #                                      engine, slots in step wait for each other's: 436 against 442 k problems/s)
        return self._replay(s, after), s

    def _load(self, s, batch):
        """Copy ``batch`` into slot ``s``'s static inputs, in front of the slot's next replay.  Returns True where the transfer was
        staged on the slot's copy stream (a pinned host arena), which is what a pair of ``lockstep`` defers its leader for."""
        dst, st = self.batches[s], self._stream(s)
        lim = ops.REQUEST_BRANCH_MAX_NODES        # the captured graph holds the one-launch GIN branch (small
        if 0 < dst.max_nodes <= lim and not 0 < batch.max_nodes <= lim:   # workflow graphs) or the layered kernels
            raise ops.GnnpnError(f"PipelinedRunner: the captured graph holds the one-launch GIN branch (graphs of <= "
                                 f"{lim} nodes); this batch has max_nodes = {batch.max_nodes}")
        packed_alike = getattr(batch, "_layout", None) is not None and batch._layout == dst._layout
        from_host = packed_alike and _pinned_host(batch._arena)
        with torch.cuda.stream(st):
            if from_host and HOST_COPY_ON_ITS_OWN_STREAM:
                # pinned host arena: the copy engine's transfer goes on a stream of its own, behind the replay that last read
                # this slot's static inputs and in front of its next one (events) — in half-batch mode the next batch then
                # crosses PCIe under the current batch's kernels
                cs = self._copy_streams[s]
                if self._slot_done[s] is not None:
                    cs.wait_event(self._slot_done[s])      # the replay that last read this slot's static inputs
                else:
                    cs.wait_stream(st)
                with torch.cuda.stream(cs):
                    dst._arena.copy_(batch._arena, non_blocking=True)
                st.wait_stream(cs)
                return True
            if from_host or (packed_alike and batch._arena.device == dst._arena.device):
                dst._arena.copy_(batch._arena, non_blocking=True)      # packed alike: one copy (device-to-device, or pinned host to device)
            else:
                for a, b in zip(self._fields(dst), self._fields(batch)):
                    if a.shape != b.shape:
                        raise ops.GnnpnError(f"PipelinedRunner: batch shape {tuple(b.shape)} != captured {tuple(a.shape)}")
                    a.copy_(b, non_blocking=True)
        return False

    def _replay(self, s, after=None):
        """One slot's replay, with the pairing of ``lockstep`` for submissions that come one at a time."""
        st, started = self._stream(s), None
        if self.lockstep:
            # A submission joins the leader that is waiting for a partner (and starts with it) if that leader has not
            # finished yet — the host runs ahead of the device, so back-to-back submissions always pair —; otherwise it
            # leads a new pair, behind whatever the other slot ran last.
            lead = self._open_leader
            if lead is not None and lead[0] != s and not lead[2].query():
                st.wait_event(lead[1])
                self._open_leader = None
            else:
                if self._last_done[1 - s] is not None:
                    st.wait_event(self._last_done[1 - s])
                started = torch.cuda.Event()
                started.record(st)
        last_held = self.common_start_us > 0 and self._hold_for_common_start(s, st)
        return self._enqueue(s, after, started, opens_gate=last_held)

    def _enqueue(self, s, after, started=None, opens_gate=False):
        """Slot ``s``'s graph replayed on its stream, ``done`` recorded behind it and booked for the slot, ``after`` called.
        ``started``: this replay leads a pair (``_replay``) that began with that event.  ``opens_gate``: this replay completes the
        burst held behind the common-start gate, which the host opens the moment the replay is enqueued."""
        st = self._stream(s)
        with torch.cuda.stream(st):
            out = self.graphs[s]()
            if opens_gate:
                self._open_gate()                   # both held replays are in their queues: they start now, together
            done = torch.cuda.Event()
            done.record(st)
            self._slot_done[s] = done               # what the next transfer into this slot's static inputs waits for
            if self.lockstep:
                self._last_done[s] = done
                if started is not None:
                    self._open_leader = (s, started, done)
            if after is not None:
                after(out, s)
        return out

    def _hold_for_common_start(self, s, st):
        """First replay after the runner was waited for: a gate (see runner_plan) in front of this replay and the other slot's next
        one.  Returns True if this replay completes the pair — the caller opens the gate once the replay is enqueued."""
        if self._gate is None and self._drained:
            # (Deliberately NOT "whenever the streams happen to be empty": a host-paced caller whose device catches up now and
            # then would pay the hold every time — measured with the pinned-host batches of tools/bench_pcie.py: -2.7 %.)
            self._gate_seq = (self._gate_seq + 1) & 0x7fffffff
            ev = torch.cuda.Event()
            with torch.cuda.stream(self._gate_stream):
                _lib.check(_lib.load().gnnpn_gate_wait(ctypes.c_void_p(self._gate_flag.data_ptr()), self._gate_seq, int(self.common_start_us),
                                                       _lib.stream_ptr()), "gnnpn_gate_wait")
                ev.record(self._gate_stream)
            self._gate = [ev, set(range(self.n_slots))]
        self._drained = False
        if self._gate is not None and s in self._gate[1]:
            st.wait_event(self._gate[0])
            self._gate[1].discard(s)
            return not self._gate[1]
        return False

    def _open_gate(self):
        """The host opens the pending gate (both replays are enqueued, or the caller is about to wait)."""
        if self._gate is not None:
            self._gate_flag[0] = self._gate_seq
            self._gate = None

    def _replay_pair(self, lead, after_lead, s, after):
        """Leader and partner enqueued together: each replay behind BOTH transfers, the leader behind whatever the partner's slot
        ran last, the partner behind the leader's start."""
        st_l, st_f = self._stream(lead), self._stream(s)
        st_l.wait_stream(self._copy_streams[s])
        st_f.wait_stream(self._copy_streams[lead])
        if self._last_done[s] is not None:
            st_l.wait_event(self._last_done[s])
        started = torch.cuda.Event()
        started.record(st_l)
        st_f.wait_event(started)
        self._enqueue(lead, after_lead)
        out = self._enqueue(s, after)
        self._open_leader = None
        return out

    def _flush_deferred(self):
        if self._deferred is not None:
            lead, after_lead = self._deferred
            self._deferred = None
            self._replay(lead, after_lead)

    def _take_turn(self):
        """Two runners of one process take TURNS on a device.  A CU holds two cooperative workgroups, which is what ONE runner's two
        launches in flight use; two runners fed alternately (two models served from one process) put four launches in front of those
        two slots, launches stay half-staffed behind each other and the bounded waits give up — loud, and very slow (round 6,
        tools/probes/dbg_two_runners.py: 200 alternating steps 3.6 s with status 0x13 against 0.11 s one runner after the other).
        So the first submit after ANOTHER runner of the device was the last to submit waits (stream-side: events, no host
        synchronisation) for everything that runner has enqueued.  Switching runners therefore drains the pipeline — a caller who
        alternates per step runs one step at a time — but every launch finds the slots it was built for."""
        import weakref
        dev = self.batches[0].x.device
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        ref = _last_runner_on_device.get(key)
        other = ref() if ref is not None else None
        if other is not self:
            if other is not None:
                other._flush_deferred()
                other._open_gate()
                for ost in other.streams:
                    ev = torch.cuda.Event()
                    ev.record(ost)
                    for st in self.streams:
                        st.wait_event(ev)
            _last_runner_on_device[key] = weakref.ref(self)

    def _stream(self, slot):
        return self.streams[slot % self.n_streams]

    def stream(self, slot):
        """The HIP stream slot ``slot``'s replays run on (half-batch mode: every slot's, there is one step in flight).  A leader
        that is waiting for its partner (``submit``) is enqueued first: work a caller puts on the stream comes behind the replay."""
        self._flush_deferred()
        return self._stream(slot)                  # (a pending common-start gate stays: it opens with the partner's replay, or by its time-out)

    def reference_run(self, slot=0):
        """The same kernels on ONE stream, nothing overlapped (used to check an overlapped result)."""
        return self.pipe.run(self.services, self.batches[slot], decode_impl=self.decode_impl, write_through=self.write_through)   # one launch per kernel, whole batch

    def _wait(self):
        """Everything this runner has been given is enqueued (a waiting leader, alone), released (a pending gate) and finished."""
        self._flush_deferred()
        self._open_gate()
        for st in self.streams:
            st.synchronize()
        self._drained = True

    def poll(self):
        """Wait for every slot's stream; the OR of the slots' sticky status words since the last poll / check, cleared — 0: no
        launch reported a failed hand-off.  The non-raising form of ``synchronize(check=True)``."""
        self._wait()
        word = 0
        for w in self.workspaces:
            word |= w.poll()
        if word:
            self._degrade(word)
        return word

    def progress(self):
        """The proof-of-work counters the last poll / synchronize read, per workspace (ops.Workspaces.last_progress)."""
        return [w.last_progress for w in self.workspaces]

    def synchronize(self, check=True):
        """Wait for every slot's stream; with ``check`` raise if any launch of any slot since the last call reported a
        failed inter-workgroup hand-off (its outputs would be garbage) — the sticky status words of the slots."""
        self._wait()
        if check:
            err = None
            for w in self.workspaces:
                try:
                    w.check("PipelinedRunner")
                except ops.GnnpnError as e:      # every workspace is read (and cleared) before the first failure is raised
                    err = err or e
            if err is not None:
                self._degrade(int(getattr(err, "status", 0xffff)))
                raise err

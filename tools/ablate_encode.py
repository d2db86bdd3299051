"""Timing experiments on the cooperative encoder (results are WRONG under ablation; timing only)."""
import sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnpn_sc_amd import ops
dev = torch.device("cuda:0")
B, L, H = 256, 235, 256
g = torch.Generator().manual_seed(0)
x = torch.rand(B, L, 8, generator=g).to(dev)
nets = []
for n in range(2):
    nets.append({"inputs": x, "w_in": ((torch.rand(4 * H, 8, generator=g) * 2 - 1) * 0.3).to(dev),
                 "b_in": ((torch.rand(4 * H, generator=g) * 2 - 1) * 0.3).to(dev),
                 "whh": ops.pack_lstm_weight((torch.rand(4 * H, H, generator=g) * 2 - 1) / 16).to(dev),
                 "bhh": ((torch.rand(4 * H, generator=g) * 2 - 1) / 16).to(dev)})
MFMA, TRANSC, SWEEP, PUBLISH = (ops.GNNPN_ABLATE_NO_MFMA, ops.GNNPN_ABLATE_NO_TRANSCENDENTALS, ops.GNNPN_ABLATE_NO_SWEEP,
                                ops.GNNPN_ABLATE_NO_PUBLISH)
def timeit(label, abl):
    ops.set_option("lstm_ablate", abl)
    for _ in range(3): ops.lstm_encode(nets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10): ops.lstm_encode(nets)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    print(f"{label:40s} ablate={abl:2d}  {ms:.3f} ms  {ms * 1e3 / L:.2f} us/step", flush=True)
timeit("full", 0)
timeit("diagnostic build, stamps on", ops.GNNPN_ABLATE_ENC_STAMPS)
timeit("full", 0)
timeit("diagnostic build, stamps on", ops.GNNPN_ABLATE_ENC_STAMPS)
timeit("no enc_out flush", ops.GNNPN_ABLATE_NO_ENC_OUT)
timeit("no input prefetch", ops.GNNPN_ABLATE_NO_INPUT_PREFETCH)
timeit("neither", ops.GNNPN_ABLATE_NO_ENC_OUT | ops.GNNPN_ABLATE_NO_INPUT_PREFETCH)
timeit("no MFMA", MFMA)
timeit("no transcendentals", TRANSC)
timeit("no MFMA, no transcendentals", MFMA | TRANSC)
timeit("no tag wait (one pass)", ops.GNNPN_ABLATE_NO_TAG_WAIT)
timeit("no sweep at all", SWEEP)
timeit("no sweep, no publish", SWEEP | PUBLISH)
timeit("no sweep/publish/MFMA", SWEEP | PUBLISH | MFMA)
timeit("no sweep/publish/MFMA/transc", SWEEP | PUBLISH | MFMA | TRANSC)
timeit("no sweep/publish/transc", SWEEP | PUBLISH | TRANSC)
ops.set_option("lstm_ablate", 0)

# phase stamps (diagnostic build path: GNNPN_ABLATE_ENC_STAMPS)
ops.set_option("lstm_ablate", ops.GNNPN_ABLATE_ENC_STAMPS)
ops.lstm_encode(nets); torch.cuda.synchronize()
ws = ops.workspaces(dev).encode()
prof = ws[32:32 + 56].view(torch.int64).cpu().tolist()
n = max(prof[5], 1)
print("flush + input prefetch part of the MFMA phase:", round(prof[6] / n))
names = ["sweep+LDS fill", "barrier 1", "A-frag reads + MFMA (+flush)", "projection + barrier 2", "cell + publish"]
print("phase cycles per step (wg 0, wave 0):", {k: round(v / n) for k, v in zip(names, prof[:5])}, "steps", n,
      "total", round(sum(prof[:5]) / n))
ops.set_option("lstm_ablate", 0)

ops.set_option("lstm_ablate", 0)
ops.lstm_encode(nets); torch.cuda.synchronize()
ws = ops.workspaces(dev).encode()
print("status", int(ws[:4].view(torch.int32).item()), "workgroups on the same-XCD fast path:", int(ws[4:8].view(torch.int32).item()))
for _ in range(3): ops.lstm_encode(nets, write_through=True)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10): ops.lstm_encode(nets, write_through=True)
e1.record(); torch.cuda.synchronize()
print(f"write-through hand-off forced: {e0.elapsed_time(e1) / 10:.3f} ms")

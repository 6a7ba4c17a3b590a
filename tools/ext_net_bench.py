#!/usr/bin/env python3
"""What a caller-supplied network costs in fused mode (Trainer.set_net_fn), one process, one MI355X: 4096 games x 400
simulations, rescnn4 with random-init weights, a warm-up generation and `reps` timed generations per line, the lines
alternating.

  builtin     fused mode with the library's rescnn4 f16x3 (set_net)
  net_fn      the same kernel through set_net_fn: the function calls Net.forward_device on the stream it is given
  torch       TorchNet with a torch-ROCm rescnn4 module (the network of tools/fit_bench.py TorchStepCnn, evaluation mode)
  compat      the reference protocol, network through net_forward (tools/run_configs.py run_compat's loop)
  compat_hc   the same with set_host_cache

usage: ext_net_bench.py [--games 4096] [--sims 400] [--reps 3] [--lines builtin,net_fn,torch,compat,compat_hc] [--out FILE.md]
Prints one JSON record per line and generation, then a markdown table (also written to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before the engine is loaded: one HIP runtime in the process (corintho_ai_amd/torch_net.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from corintho_ai_amd import NET_RESCNN4_H3, Trainer, nets  # noqa: E402
from corintho_ai_amd.net import Net  # noqa: E402

SPE = 16


def torch_rescnn4(w, device):
    """rescnn4 in torch-ROCm, inference: tools/fit_bench.py TorchStepCnn's graph with the moving statistics"""
    F = torch.nn.functional

    class ResCnn4(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for name, a in nets.rescnn4_unpack(w).items():
                t = torch.tensor(a)
                if a.ndim == 4:
                    t = t.permute(3, 2, 0, 1).contiguous()  # HWIO -> OIHW
                elif name in ("p_k", "v_k"):
                    t = t.t().contiguous().view(a.shape[1], a.shape[0], 1, 1)
                self.register_buffer(name, t)

        def cbr(self, x, pre, pad, res=None):
            g = lambda k: getattr(self, pre + k)  # noqa: E731
            z = F.conv2d(x, g("_k"), g("_b"), padding=pad)
            y = g("_bn0").view(1, -1, 1, 1) * ((z - g("_bn2").view(1, -1, 1, 1)) * torch.rsqrt(g("_bn3").view(1, -1, 1, 1) + 1e-3)) \
                + g("_bn1").view(1, -1, 1, 1)
            return torch.relu(y if res is None else y + res)

        def forward(self, s):
            n = s.shape[0]
            x = torch.cat([s[:, :64].view(n, 16, 4), s[:, None, 64:70].expand(n, 16, 6)], 2).view(n, 4, 4, 10).permute(0, 3, 1, 2)
            h = self.cbr(x, "stem", 1)
            for b in range(4):
                h = self.cbr(self.cbr(h, "b%d_c1" % b, 1), "b%d_c2" % b, 1, res=h)
            pa = self.cbr(h, "p", 0).permute(0, 2, 3, 1).reshape(n, 64)
            va = self.cbr(h, "v", 0).permute(0, 2, 3, 1).reshape(n, 32)
            v = (torch.relu(va @ self.v_d1k + self.v_d1b) @ self.v_d2k).view(-1) + self.v_d2b
            return torch.tanh(v), torch.softmax(pa @ self.p_dk + self.p_db, 1)

    return ResCnn4().to(device).eval()


class Line:
    """one way to play a generation: play(seed) -> the rows the caller's function was asked for (None: no function)"""

    def __init__(self, name, G, S, w):
        self.name, self.G = name, G
        self.t = Trainer(G, "", 12345, S, SPE, 1.0, 0.25, 0, 1, False, stagger=False)
        self.asked = 0
        self.keep = []
        getattr(self, "setup_" + name)(w)

    def setup_builtin(self, w):
        self.t.set_net(NET_RESCNN4_H3, w)

    def setup_net_fn(self, w):
        rows = self.t.request_rows()
        st = torch.zeros((rows, 70), dtype=torch.float32, device="cuda")
        ev = torch.zeros(rows, dtype=torch.float32, device="cuda")
        pr = torch.zeros((rows, 96), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        net = Net(NET_RESCNN4_H3, w, rows)
        ps, pe, pp = st.data_ptr(), ev.data_ptr(), pr.data_ptr()

        def fn(row0, cap, d_rows, stream):
            self.asked += cap
            net.forward_device(ps + row0 * 280, cap, d_rows, pe + row0 * 4, pp + row0 * 384, stream)

        self.keep = [st, ev, pr, net]
        self.t.set_net_fn(fn, ps, pe, pp, rows, flop_per_row=nets.rescnn4_flop_per_row())

    def setup_torch(self, w):
        from corintho_ai_amd.torch_net import TorchNet

        self.keep = [TorchNet(torch_rescnn4(w, "cuda"), self.t, flop_per_row=nets.rescnn4_flop_per_row())]

    def setup_compat(self, w):
        self.t.set_net(NET_RESCNN4_H3, w)
        cap = self.G * SPE
        self.arrays = (np.zeros(cap, np.float32), np.zeros((cap, 96), np.float32), np.zeros((cap, 70), np.float32))
        self.t.pin(*self.arrays)

    def setup_compat_hc(self, w):
        self.setup_compat(w)
        self.t.set_host_cache(True)

    def play(self, seed):
        t = self.t
        t.reset(seed)
        self.asked = 0
        if self.keep and hasattr(self.keep[0], "rows_asked"):
            self.keep[0].rows_asked = 0
        t0 = time.perf_counter()
        if self.name.startswith("compat"):
            evals, probs, gs = self.arrays
            while not t.doIteration(evals, probs, -1):
                n = t.num_requests(-1)
                if n:
                    t.writeRequests(gs, -1)
                    t.net_forward(gs[:n], out_evals=evals, out_probs=probs)
        else:
            assert t.run()
        dt = time.perf_counter() - t0
        st = t.stats()
        asked = self.keep[0].rows_asked if self.keep and hasattr(self.keep[0], "rows_asked") else self.asked
        return {"line": self.name, "seconds": dt, "games_per_s": self.G / dt, "iterations": st["iterations"], "nn_rows": st["nn_rows"],
                "nn_rows_evaluated": st["nn_rows_evaluated"], "rows_asked": asked or None, "pools": st["pools"], "resident_slots": st["resident_slots"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lines", default="builtin,net_fn,torch,compat,compat_hc")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    w = nets.init_rescnn4(0)
    lines = [Line(name, a.games, a.sims, w) for name in a.lines.split(",")]
    for ln in lines:  # warm-up
        print(json.dumps(dict(ln.play(1), warmup=True)), flush=True)
    recs = {ln.name: [] for ln in lines}
    for r in range(a.reps):
        for ln in lines:
            rec = ln.play(100 + r)
            recs[ln.name].append(rec)
            print(json.dumps(rec), flush=True)
    head = "| line | games/s | s per generation (each) | iterations | nn_rows | nn_rows_evaluated | rows the function was asked for |\n|---|---|---|---|---|---|---|\n"
    body = ""
    for name, rs in recs.items():
        m = lambda k: sum(x[k] for x in rs) / len(rs)  # noqa: E731
        body += "| %s | %.0f | %.3f (%s) | %.0f | %.0f | %.0f | %s |\n" % (
            name, a.games / m("seconds"), m("seconds"), " ".join("%.3f" % x["seconds"] for x in rs), m("iterations"), m("nn_rows"),
            m("nn_rows_evaluated"), "%.0f" % m("rows_asked") if rs[0]["rows_asked"] else "-")
    table = "%d games x %d simulations, searches_per_eval %d, rescnn4 (random init), means of %d generations\n\n%s%s" % (
        a.games, a.sims, SPE, a.reps, head, body)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table)


if __name__ == "__main__":
    main()

"""Time the flow-statistics stage (stts_flow_stats_forward: cond, eight coupling layers on three streams) per direction and write
profiles/flow_stats_bench.txt.  Shapes: 1 x 3 s, 8 x 3 s, 16 x 10 s.  Per shape and direction: every form forced (STTS_FSTAT_WN = 0: plain
contractions and the coupling row kernel, 88 launches; 16 / 32 / 64: wn_stats_kernel, 32 launches, on that block height), the plan's own choice, and
the same network in torch eager fp32 on the same GPU (written here: conv1d / linear with the folded weights).  Alongside, as context, the engine's
prior_flow stage at STTS_PREC_F32_NATIVE: the same WaveNet work on the same matrix cores with the F(M,5) forms and one stream (plus the prior and
post_flow).  The forms alternate inside one process, round after round, so that drift of the box shows as spread and not as a difference; every figure
is the median over the rounds of a window of CALLS calls between two events on the stream, with min .. max behind it.
usage: python tools/flow_stats_bench.py [--rounds 7] [--calls 20] [--shapes 1x960,8x960,16x3200] [--out profiles/flow_stats_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

entry.compile()  # before the GPU is touched
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stylish_tts_amd import params, synth  # noqa: E402
from stylish_tts_amd.config import load_model_config  # noqa: E402
from stylish_tts_amd.runtime import HipModel, Segments  # noqa: E402

W_FLOW_STATS = 524288
FORMS = ("0", "16", "32", "64", None)  # None: the plan's choice


class Eager(torch.nn.Module):
    """ResidualCouplingBlock.forward with three streams (models/flow.py:132-151, :196-218) in torch eager, weights folded once; [B, 128, T] each."""

    def __init__(self, w, dev):
        super().__init__()
        t = lambda k: torch.from_numpy(np.asarray(w[k], np.float32)).to(dev)  # noqa: E731
        wn = lambda p: torch._weight_norm(t(p + ".weight_v"), t(p + ".weight_g"), 0)  # noqa: E731
        self.layers = []
        for f in range(8):
            q = f"flow.flows.{2 * f}."
            self.layers.append(dict(pre=(t(q + "pre.weight"), t(q + "pre.bias")), cond=(wn(q + "enc.cond_layer").reshape(1024, -1), t(q + "enc.cond_layer.bias")),
                                    inw=[(wn(q + f"enc.in_layers.{i}"), t(q + f"enc.in_layers.{i}.bias")) for i in range(4)],
                                    rs=[(wn(q + f"enc.res_skip_layers.{i}"), t(q + f"enc.res_skip_layers.{i}.bias")) for i in range(4)],
                                    pm=(t(q + "proj_mean.weight"), t(q + "proj_mean.bias")), pl=(t(q + "proj_logstd.weight"), t(q + "proj_logstd.bias"))))

    @torch.no_grad()
    def forward(self, z, mean, logstd, style, reverse):
        F = torch.nn.functional
        three = [list(torch.split(a, 64, 1)) for a in (z, mean, logstd)]
        for f in (reversed(range(8)) if reverse else range(8)):
            L = self.layers[f]
            if reverse:
                three = [[b, a] for a, b in three]
            h = F.linear(three[0][0].mT, *L["pre"]).mT
            g = F.linear(style, *L["cond"])[:, :, None]
            out = torch.zeros_like(h)
            for i in range(4):
                a = F.conv1d(h, *L["inw"][i], padding=2) + g[:, i * 256 : (i + 1) * 256]
                rs = F.linear((torch.tanh(a[:, :128]) * torch.sigmoid(a[:, 128:])).mT, *L["rs"][i]).mT
                if i < 3:
                    h = h + rs[:, :128]
                    out = out + rs[:, 128:]
                else:
                    out = out + rs
            m, s = F.linear(out.mT, *L["pm"]).mT, F.linear(out.mT, *L["pl"]).mT
            if reverse:
                three = [[three[0][0], (three[0][1] - m) * torch.exp(-s)], [three[1][0], (three[1][1] - m) * torch.exp(-s)], [three[2][0], three[2][1] - s]]
            else:
                three = [[three[0][0], m + three[0][1] * torch.exp(s)], [three[1][0], m + three[1][1] * torch.exp(s)], [three[2][0], three[2][1] + s]]
                three = [[b, a] for a, b in three]
        return [torch.cat(p, 1) for p in three]


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="1x960,8x960,16x3200")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flow_stats_bench.txt"))
    ap.add_argument("--only", default=None, help="one form only, both directions (a profiler run): 0 | 16 | 32 | 64 | plan")
    a = ap.parse_args()
    entry.load()
    cfg = load_model_config()
    w = params.synth_state_dict(params.speech_predictor_spec(cfg), 0, prefix="speech_predictor.")
    m = HipModel(cfg, 0)
    m.load_state_dict("speech_predictor", w)
    m.finalize(W_FLOW_STATS)
    native = None
    if a.only is None:
        native = HipModel(cfg, 0, precision="f32_native")
        native.load_state_dict("speech_predictor", w)
        native.finalize(7)
    eager = Eager(w, m.device)
    lines = [f"flow_stats_bench: {a.rounds} rounds x {a.calls} calls per window, forms alternated per round; ms per call: median (min .. max)"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(m.device)  # noqa: E731
    for shape in a.shapes.split(","):
        B, T4 = (int(v) for v in shape.split("x"))
        seg, R = Segments([T4] * B, m.device), B * T4
        mean = dev(0.5 * synth.normal("fsb.mean", (R, 128)))
        logstd = dev(0.3 * synth.normal("fsb.logstd", (R, 128)) - 0.5)
        z = mean + dev(synth.normal("fsb.eps", (R, 128))) * torch.exp(logstd)
        style = dev(0.5 * synth.normal("fsb.style", (B, 64)))
        bct = [t.reshape(B, T4, 128).transpose(1, 2).contiguous() for t in (z, mean, logstd)]
        x = dev(synth.normal("fsb.x", (R, cfg.decoder.hidden_dim)))

        def stage(form, reverse):
            def run():
                if form is None:
                    os.environ.pop("STTS_FSTAT_WN", None)
                else:
                    os.environ["STTS_FSTAT_WN"] = form
                m.flow_stats(seg, z, mean, logstd, style, reverse)
            return run

        jobs = {}
        for reverse in (False, True):
            d = "reverse" if reverse else "forward"
            for f in FORMS:
                if a.only is None or f == (None if a.only == "plan" else a.only):
                    jobs[f"{d} " + ("form " + f if f is not None else "plan")] = stage(f, reverse)
            if a.only is None:
                jobs[f"{d} torch eager"] = (lambda rv: lambda: eager(*bct, style, rv))(reverse)
        if native is not None:
            jobs["prior_flow f32_native"] = lambda: native.prior_flow(seg, x, style, z)
        for fn in jobs.values():  # warm-up: every form at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in jobs}
        for _ in range(a.rounds):
            for k, fn in jobs.items():
                times[k].append(window_ms(fn, a.calls))
        os.environ.pop("STTS_FSTAT_WN", None)
        lines.append(f"{B} x {T4 * m.hop4 / cfg.sample_rate:g} s ({R} rows)")
        for k, v in times.items():
            lines.append(f"  {k:24s} {statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})")
        print("\n".join(lines[-len(times) - 1 :]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Time the posterior-encoder stage (stts_posterior_forward: STFT, two pre contractions, cond, 12 WaveNet layers, the projection, post_flow) and
the resynthesis call, and write profiles/posterior_bench.txt.  Shapes: 1 x 3 s, 8 x 3 s, 16 x 10 s of audio.  Per shape: every WaveNet form forced
(STTS_POST_WN = 0: plain contractions, 24 launches; 16 / 32 / 64: wn_post_kernel, one launch per layer, on that block height), the plan's own choice,
Synthesizer.resynthesize end to end, and a torch-eager restatement of PosteriorEncoder on the same GPU (written here: rocFFT STFT, conv1d / linear with
the folded weights).  The forms alternate inside one process, round after round, so that drift of the box shows as spread and not as a difference;
every figure is the median over the rounds of a window of CALLS calls between two events on the stream, with min .. max behind it.
usage: python tools/posterior_bench.py [--rounds 7] [--calls 20] [--shapes 1x960,8x960,16x3200] [--out profiles/posterior_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

entry.compile()  # before the GPU is touched
import numpy as np  # noqa: E402
import torch  # noqa: E402

from stylish_tts_amd import params, pipeline, synth  # noqa: E402
from stylish_tts_amd.config import load_model_config  # noqa: E402
from stylish_tts_amd.runtime import HipModel, Segments  # noqa: E402

W_POSTERIOR = 262144
FORMS = ("0", "16", "32", "64", None)  # None: the plan's choice


class Eager(torch.nn.Module):
    """PosteriorEncoder.forward (models/flow.py:282-293) in torch eager, weights folded once; x [B, S] -> z [B, 128, T]."""

    def __init__(self, sd, cfg, dev):
        super().__init__()
        t = lambda k: torch.from_numpy(np.asarray(sd[k], np.float32)).to(dev)  # noqa: E731
        wn = lambda p: torch._weight_norm(t(p + ".weight_v"), t(p + ".weight_g"), 0)  # noqa: E731
        self.n_fft, self.win, self.hop = cfg.n_fft, cfg.win_length, cfg.hop_length // 4
        self.window = torch.hann_window(self.win, device=dev)
        self.pre = [(t(f"pre_{n}.weight"), t(f"pre_{n}.bias")) for n in ("spec", "phase")]
        self.win_w = [(wn(f"enc.in_layers.{i}"), t(f"enc.in_layers.{i}.bias")) for i in range(12)]
        self.rs_w = [(wn(f"enc.res_skip_layers.{i}"), t(f"enc.res_skip_layers.{i}.bias")) for i in range(12)]
        self.cond = (wn("enc.cond_layer"), t("enc.cond_layer.bias"))
        self.pm, self.pl = (t("proj_mean.weight"), t("proj_mean.bias")), (t("proj_logstd.weight"), t("proj_logstd.bias"))

    @torch.no_grad()
    def forward(self, x, style, noise):
        F = torch.nn.functional
        X = torch.stft(x, self.n_fft, self.hop, self.win, window=self.window, return_complex=True)[:, :, :-1]
        h = torch.cat([F.conv1d(X.abs(), *self.pre[0]), F.conv1d(torch.angle(X), *self.pre[1])], dim=1)
        g = F.linear(style, *self.cond)[:, :, None]
        out = torch.zeros_like(h)
        for i in range(12):
            a = F.conv1d(h, *self.win_w[i], padding=1) + g[:, i * 256 : (i + 1) * 256]
            acts = torch.tanh(a[:, :128]) * torch.sigmoid(a[:, 128:])
            rs = F.linear(acts.mT, *self.rs_w[i]).mT
            if i < 11:
                h = h + rs[:, :128]
                out = out + rs[:, 128:]
            else:
                out = out + rs
        mean, logstd = F.linear(out.mT, *self.pm).mT, F.linear(out.mT, *self.pl).mT
        return mean + noise * torch.exp(logstd)


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "posterior_bench.txt"))
    ap.add_argument("--only", default=None, help="one form only (a profiler run): 0 | 16 | 32 | 64 | plan")
    a = ap.parse_args()
    entry.load()
    cfg = load_model_config()
    sd = params.synth_state_dict(params.posterior_encoder_spec(cfg, ""), 0, prefix="speech_predictor.posterior_encoder.")
    m = HipModel(cfg, 0)
    m.load_state_dict("speech_predictor", params.synth_state_dict(params.speech_predictor_spec(cfg), 0, prefix="speech_predictor."))
    m.load_state_dict("speech_predictor", sd, prefix="posterior_encoder.")
    m.finalize(15 | W_POSTERIOR)
    eager = Eager(sd, cfg, m.device)
    syn = pipeline.Synthesizer(m)
    lines = [f"posterior_bench: {a.rounds} rounds x {a.calls} calls per window, forms alternated per round; ms per call: median (min .. max)"]
    for shape in a.shapes.split(","):
        B, T4 = (int(v) for v in shape.split("x"))
        seg, R, h = Segments([T4] * B, m.device), B * T4, m.hop4
        wave = torch.from_numpy((0.3 * synth.normal("pb.wave", (R * h,))).astype(np.float32)).to(m.device)
        style = torch.from_numpy((0.5 * synth.normal("pb.style", (B, 64))).astype(np.float32)).to(m.device)
        noise = torch.from_numpy(synth.normal("pb.noise", (R, 128)).astype(np.float32)).to(m.device)
        noise_bct = noise.reshape(B, T4, 128).transpose(1, 2).contiguous()
        T = T4 // 4
        toks = [[int(v) for v in synth.tokens("pb.tok", 1, 40, 178)[0]] for _ in range(B)]
        durs = [synth.durations_for(f"pb.dur{b}", 40, T) for b in range(B)]
        f0 = [torch.full((T,), 150.0) for _ in range(B)]
        rz = dict(posterior_noise=noise, src_noise=torch.from_numpy(synth.normal("pb.sn", (R * h,)).astype(np.float32)).to(m.device), init_phase=torch.tensor([0.3], device=m.device))

        def stage(form):
            def run():
                if form is None:
                    os.environ.pop("STTS_POST_WN", None)
                else:
                    os.environ["STTS_POST_WN"] = form
                m.posterior(seg, audio=wave, style=style, noise=noise, mel=True, stats=False)
            return run

        jobs = {("form " + f if f is not None else "plan"): stage(f) for f in FORMS}
        if a.only is not None:
            jobs = {k: v for k, v in jobs.items() if k == ("plan" if a.only == "plan" else "form " + a.only)}
        else:
            jobs["resynthesize"] = lambda: syn.resynthesize(toks, [wave[b * T4 * h : (b + 1) * T4 * h] for b in range(B)], durs, f0, noise=rz)
            jobs["torch eager"] = lambda: eager(wave.reshape(B, T4 * h), style, noise_bct)
        for fn in jobs.values():  # warm-up: every form at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in jobs}
        for _ in range(a.rounds):
            for k, fn in jobs.items():
                times[k].append(window_ms(fn, a.calls))
        os.environ.pop("STTS_POST_WN", None)
        lines.append(f"{B} x {T4 * h / cfg.sample_rate:g} s ({R} rows)")
        for k, v in times.items():
            lines.append(f"  {k:14s} {statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})")
        print("\n".join(lines[-len(times) - 1 :]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

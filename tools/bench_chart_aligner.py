"""Times ONE WHOLE ITERATION of the chart alignment (g4splat_amd/chart_aligner.py) -- confidence, deformation, alignment and
matching losses, weighted sum, backward, Adam step, zero grads -- at n = 5, 20 and 50 charts of 384 x 512 (--sizes), with the loss
flags and weights of the `strong` and of the `default` configuration (chart_aligner.ALIGNMENT_CONFIGS), in three variants:

  graph   ChartAligner with the iteration captured in a HIP graph: one graph launch per iteration
  eager   ChartAligner, the same iteration launched from Python
  parent  what could be composed before ChartAligner existed: ChartDeformation.deformed_depths() + AlignmentLosses.terms +
          ChartMatcher.loss + the regularisers and the confidence activation as torch ops + torch.optim.Adam(eps=1e-15).
          For `strong` ChartDeformation cannot weight the encodings, so this variant applies the confidence weighting on a plain
          torch restatement of the deformation (four grid_sample calls, a cat, the weighting, the depth encoding's grid_sample,
          three bmm; written here from the contract as in tools/bench_chart_deform.py) and takes the norm term from the same
          sampled encodings -- the reference samples them a second time, so this side is if anything cheaper than the stage it
          stands for.

Scene: tools/bench_chart_match.py's (views on an arc at a slanted plane, 3 % noise); the reference depths are the initial ones
with a smooth 0.5 % bump.  Every variant starts from the same seeded prepare_for_optimization; before timing, the first loss of
the three variants is compared (1e-4 of its value: the `strong` parent side is another float32 evaluation).  Timing: each round
runs --iters iterations of one variant between two device synchronisations, --warmup warm-up rounds, then --rounds rounds that
alternate the variants; medians (min .. max) of the per-iteration time.  The allocator peak is torch's above what is held before
the round; a graph replay allocates nothing (its working set, the eager variant's, lies in the graph's pool), so for that variant
what stays allocated after the capture (the graph's outputs and the optimiser's moments, created in its warm-up) is reported.  --launches counts the device kernels of one iteration with torch.profiler (eager and parent; a graph replay is one
launch from the host, its kernel nodes are the eager variant's).

    python tools/bench_chart_aligner.py [--sizes 5,20,50] [--rounds 5] [--warmup 2] [--iters 10] [--launches] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from g4splat_amd import _lib, chart_align, chart_aligner, chart_deform, chart_match  # noqa: E402
from tools.bench_chart_match import DEV, alternate, make_scene  # noqa: E402

OPTIMIZE_KEYS = ("use_gradient_loss", "use_hessian_loss", "use_normal_loss", "use_curvature_loss", "use_matching_loss",
                 "use_confidence_in_matching_loss", "gradient_loss_weight", "hessian_loss_weight", "normal_loss_weight",
                 "curvature_loss_weight", "matching_loss_weight", "encodings_lr", "mlp_lr", "confidence_lr",
                 "regularize_chart_encodings_norms", "chart_encodings_norm_loss_weight", "use_total_variation_on_depth_encodings",
                 "total_variation_on_depth_encodings_weight")


def torch_weighted_depths(m, params, w):
    """(depths, enc) of the contract in plain torch (tools/bench_chart_deform.py torch_depths) with the chart encoding weighted"""
    n, H, W = m.n, m.height, m.width
    lin = lambda K: torch.linspace(-1.0, 1.0, K, device=DEV)  # noqa: E731
    uv = torch.stack(torch.meshgrid(lin(H), lin(W), indexing="ij"), dim=-1).repeat(n, 1, 1, 1)
    levels = [p for k, p in params.items() if k.startswith("charts_encoding")]
    enc = torch.cat([torch.nn.functional.grid_sample(v, uv, mode="bilinear", padding_mode="border", align_corners=False).permute(0, 2, 3, 1)
                     for v in levels], dim=-1).reshape(n, H * W, -1)
    x = enc * w.reshape(n, H * W, 1)
    grid = torch.cat([torch.zeros(n, H * W, 1, 1, device=DEV), -1 + 2 * m.depth_coords.view(n, H * W, 1, 1)], dim=-1)
    denc = torch.nn.functional.grid_sample(params["depth_encoding.encodings"][..., None], grid, mode="bilinear", padding_mode="border",
                                           align_corners=False)[..., 0].permute(0, 2, 1)
    x = (x + denc) / m.scene_radius
    for j in range(m._NL):
        x = torch.bmm(x, params[f"deformation.mlp.{2 * j}.weight"].transpose(1, 2)) + params[f"deformation.mlp.{2 * j}.bias"][:, None, :]
        if j < m._NL - 1:
            x = torch.relu(x)
    delta = (x[..., 0] * m.deformation_radius).reshape(n, H, W)
    y, xx = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    pix = torch.stack([xx, y, torch.ones_like(xx)], -1).reshape(1, H * W, 3)
    dirs = pix @ m._cams[:, 3:12].reshape(n, 3, 3).transpose(1, 2)
    return m._d0 + delta * (torch.sign(m._d0) / dirs.norm(dim=-1).reshape(n, H, W)), enc


class Parent:
    """The parent commit's composition of one iteration, on its own ChartDeformation, confidence and torch.optim.Adam."""

    def __init__(self, cams, d0, reference, cfg, matching_thr, state):
        self.cfg, self.reference = cfg, reference
        self.m = chart_deform.ChartDeformation(cams, d0)
        self.m.load_state_dict({k: v for k, v in state.items() if k != "_confidence"})
        self.raw = torch.nn.Parameter(state["_confidence"].clone())
        self.losses = chart_align.AlignmentLosses(cams, d0, 0.2)
        self.matcher = chart_match.ChartMatcher(cams, reference_depths=reference)
        self.matcher.match(matching_thr)
        named = dict(self.m.named_parameters())
        groups = [{"params": [p], "lr": cfg["encodings_lr"], "name": k} for k, p in named.items() if k.endswith("encodings")]
        groups.append({"params": [self.raw], "lr": cfg["confidence_lr"], "name": "_confidence"})
        groups += [{"params": [p], "lr": cfg["mlp_lr"], "name": k} for k, p in named.items() if not k.endswith("encodings")]
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        self.weights = {"gradient": cfg["gradient_loss_weight"] if cfg["use_gradient_loss"] else None,
                        "normal": cfg["normal_loss_weight"] if cfg["use_normal_loss"] else None,
                        "curvature": cfg["curvature_loss_weight"] if cfg["use_curvature_loss"] else None,
                        "matching": cfg["matching_loss_weight"] if cfg["use_matching_loss"] else None,
                        "norm": cfg["chart_encodings_norm_loss_weight"] if cfg["regularize_chart_encodings_norms"] else None,
                        "tv": cfg["total_variation_on_depth_encodings_weight"] if cfg["use_total_variation_on_depth_encodings"] else None}

    def iteration(self):
        cfg, m = self.cfg, self.m
        conf = 1.0 + torch.exp(self.raw)
        zero = torch.zeros((), device=DEV)
        reg = [zero, zero]
        if cfg["weight_encodings_with_confidence"]:
            w = 1.0 - torch.exp(-(conf.detach() - 1.0) ** 2 / 2)
            depths, enc = torch_weighted_depths(m, dict(m.named_parameters()), w)
            if cfg["regularize_chart_encodings_norms"]:
                reg[0] = enc.norm(dim=-1).mean()
        else:
            depths = m.deformed_depths()
        if cfg["use_total_variation_on_depth_encodings"]:
            q = m.depth_encoding.encodings
            reg[1] = (q[..., 1:] - q[..., :-1]).abs().mean()
        terms = self.losses.terms(depths, self.reference, conf, None, None, cfg["use_gradient_loss"], cfg["use_normal_loss"],
                                  cfg["use_curvature_loss"])
        matching = self.matcher.loss(depths) if cfg["use_matching_loss"] else None
        loss = chart_aligner.total_loss(terms, reg, matching, self.weights)
        loss.backward()
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        return loss.detach()


def count_kernels(fn):
    """The device kernels of one call of fn, by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize(DEV)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(DEV)
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5,20,50")
    ap.add_argument("--flavours", default="strong,default")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    result = {"build_id": _lib.load().g4s_version().decode(), "device": torch.cuda.get_device_name(DEV), "rounds": a.rounds,
              "warmup": a.warmup, "iters": a.iters, "height": H, "width": W}
    rows = []
    for n in (int(s) for s in a.sizes.split(",")):
        cams, d0, reference = make_scene(n, H, W, noise=0.03)
        for flavour in a.flavours.split(","):
            cfg = chart_aligner.ALIGNMENT_CONFIGS[flavour]
            kw = {k: cfg[k] for k in OPTIMIZE_KEYS}
            aligners = {}
            for variant in ("graph", "eager"):
                al = chart_aligner.ChartAligner(cams, d0, weight_encodings_with_confidence=cfg["weight_encodings_with_confidence"])
                torch.manual_seed(11)
                al.optimize(reference, n_iterations=0, graph=variant == "graph", lr_update_iters=[], **kw)  # set up, no iteration
                aligners[variant] = al
            state = {k: v.detach().clone() for k, v in aligners["eager"].state_dict().items()}
            thr = chart_match.MATCHING_THR_FACTOR * aligners["eager"]._spatial_extent
            parent = Parent(cams, d0, reference, cfg, thr, state)
            g_al, e_al = aligners["graph"], aligners["eager"]
            torch.cuda.synchronize(DEV)
            held = torch.cuda.memory_allocated(DEV)
            graph, (g_vec, _d) = g_al._capture(g_al._options)
            torch.cuda.synchronize(DEV)
            pool_mib = (torch.cuda.memory_allocated(DEV) - held) / 2 ** 20  # live after the capture: its outputs, the optimiser's moments

            def run_graph():
                for _ in range(a.iters):
                    graph.replay()
                return g_vec

            def run_eager():
                for _ in range(a.iters):
                    out = e_al._iteration(e_al._options)[0]
                return out

            def run_parent():
                for _ in range(a.iters):
                    out = parent.iteration()
                return out

            graph.replay()
            first = {"graph": float(g_vec[0]), "eager": float(e_al._iteration(e_al._options)[0][0]), "parent": float(parent.iteration())}
            assert first["graph"] == first["eager"], first
            assert abs(first["parent"] - first["eager"]) <= 1e-4 * abs(first["eager"]), first
            launches = None
            if a.launches:
                launches = {"eager": count_kernels(lambda: e_al._iteration(e_al._options)), "parent": count_kernels(parent.iteration)}
            sides = {"graph": run_graph, "eager": run_eager, "parent": run_parent}
            t = alternate(sides, a.rounds, a.warmup)
            per = {k: tuple(x / a.iters for x in v[:3]) + (v[3],) for k, v in t.items()}
            row = f"n = {n:2d} {flavour:7s}: " + " | ".join(
                f"{k} {per[k][0]:8.3f} ms ({per[k][1]:.3f} .. {per[k][2]:.3f}) {per[k][3]:8.1f} MiB" for k in sides)
            row += f" | parent / graph x{per['parent'][0] / per['graph'][0]:.2f}, eager / graph x{per['eager'][0] / per['graph'][0]:.2f}"
            row += (f" | after the capture {pool_mib:.1f} MiB stay allocated (the graph's outputs and the optimiser's moments); a replay "
                    "allocates nothing, its working set is the eager variant's, kept in the graph's pool")
            if launches:
                row += f" | kernels per iteration: eager (= the graph's nodes) {launches['eager']}, parent {launches['parent']}; graph launches 1"
            rows.append(row)
            print(row, flush=True)
            result[f"n_{n}_{flavour}"] = {k: {"ms": per[k][0], "min": per[k][1], "max": per[k][2], "mib": per[k][3]} for k in sides}
            result[f"n_{n}_{flavour}"]["first_loss"] = first
            result[f"n_{n}_{flavour}"]["graph_held_mib"] = pool_mib
            if launches:
                result[f"n_{n}_{flavour}"]["kernels"] = launches
            del aligners, parent, graph, g_al, e_al
            torch.cuda.empty_cache()
    text = "\n".join([f"{result['build_id']} on {result['device']}; per-iteration medians (min .. max) of {a.rounds} alternating rounds of "
                      f"{a.iters} iterations after {a.warmup} warm-ups"] + rows)
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(result) + "\n")


if __name__ == "__main__":
    main()

"""MAE-pretrain throughput benchmark on MI355X (BASELINE.json metric), one process per GPU.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" is one optimisation step of the reference harness (``cinema/mae/pretrain.py:242-269``) on one synthetic
minibatch that is already resident in HBM: forward (random 75 % masks) + backward + [gradient all-reduce] + global-norm
clip + AdamW + zero_grad.  Workload = BASELINE.json configs[1]: CineMA ViT-Base, 4 views (SAX 192x192x16 + 3 LAX 192x192),
per-GPU batch 16, bf16 MFMA compute with fp32 accumulation / residual stream / master weights.  Weak scaling: the per-GPU
batch is fixed, ``value`` is the whole-job samples/s.

Rank 0 prints ONE JSON line with the extra ``roofline`` (dominant kernel, live HIP-event timing of every GEMM launch on
the launch stream during extra instrumented steps) and ``cpu_baseline`` (the CPU oracle timed on the host cores) objects; the
per-kernel tables and the secondary configurations' details go to ``--details FILE`` only.  ``--dump-outputs DIR`` writes what the
last timed step returned as ``.npy`` files.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

STEP_GFLOP_PER_SAMPLE = 835.0  # 3 x 278.4 GF forward, reference graph, no recompute credit
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0           # HBM3E, same guide (about 6.3 TB/s is what a streaming kernel can reach)
RIDGE_FLOP_PER_BYTE = MFMA_BF16_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9)  # 312.5: below it the HBM roof is the one that applies


def gemm_roof(flops: float, alg_bytes: float, secs: float, peak_tflops: float = MFMA_BF16_PEAK_TFLOPS) -> dict:
    """Which roof applies to a GEMM instance and how far below it the instance runs: intensity = algorithmic FLOP / algorithmic byte (every operand read once,
    the result written once, epilogue tensors included); below the ridge (peak FLOP/s / 8 TB/s) the attainable rate is intensity x 8 TB/s, i.e. the kernel is
    priced against the HBM roof and ``frac`` = algorithmic bytes / time / 8 TB/s; above it against the MFMA peak."""
    ridge = peak_tflops * 1e12 / (HBM_PEAK_GBS * 1e9)
    inten = flops / max(alg_bytes, 1.0)
    tf, gbs = flops / secs / 1e12, alg_bytes / secs / 1e9
    hbm = inten < ridge
    return {"bound": "hbm" if hbm else "mfma", "intensity_flop_per_byte": round(inten, 1), "tflops": round(tf, 1), "alg_gb_s": round(gbs, 1),
            "frac": round(gbs / HBM_PEAK_GBS if hbm else tf / peak_tflops, 4), "frac_of_mfma_peak": round(tf / peak_tflops, 4)}


def hipblaslt_reference(prof: list, steps: int, names: dict) -> dict:
    """MEASUREMENT ONLY (the library never calls a BLAS): for every GEMM instance of the profiled steps, the time hipBLASLt (through ``torch.mm``) takes for the same
    problems - same m, n, k, same operand layouts in memory, bf16 operands and a bf16 result, NO epilogue, one call per problem back to back on an otherwise idle
    chip - next to the time this library's launches took inside the step (which includes their fused epilogues: bias, GELU, residual, fp32 accumulation, bias-gradient
    row sums).  ``vs_hipblaslt`` = hipBLASLt time / this library's time (> 1: faster than the vendor GEMM on these shapes).  e4m3 instances are skipped."""
    import torch
    from collections import Counter

    per_kind: dict = {}
    for kind, _f, _e0, _e1, _shape, *rest in prof:
        if kind >= 4096 or not rest:  # e4m3 weight gradients: no bf16 BLAS equivalent of the same bytes
            continue
        per_kind.setdefault(kind, Counter()).update(rest[0])
    shapes = sorted({s for c in per_kind.values() for s in c})
    t_us: dict = {}
    for m, n, k, akm, bkm in shapes:
        try:
            a = torch.randn((m, k) if akm else (k, m), device="cuda").mul_(0.5).to(torch.bfloat16)
            b = torch.randn((n, k) if bkm else (k, n), device="cuda").mul_(0.05).to(torch.bfloat16)
            av, bv = (a if akm else a.t()), (b.t() if bkm else b)
            y = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
            for _ in range(3):
                torch.mm(av, bv, out=y)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(8):
                torch.mm(av, bv, out=y)
            e1.record()
            torch.cuda.synchronize()
            t_us[(m, n, k, akm, bkm)] = e0.elapsed_time(e1) / 8 * 1e3
            del a, b, y
        except RuntimeError:
            t_us[(m, n, k, akm, bkm)] = None
    ours: dict = {}  # (kind, problem) -> [seconds, launches] of the single-problem launches (a grouped launch has one time for all its problems)
    ours_kind: dict = {}
    for kind, _f, e0, e1, _shape, *rest in prof:
        if kind in per_kind:
            dt = e0.elapsed_time(e1) * 1e-3
            ours_kind[kind] = ours_kind.get(kind, 0.0) + dt
            if len(rest[0]) == 1:
                o = ours.setdefault((kind, rest[0][0]), [0.0, 0])
                o[0] += dt
                o[1] += 1
    out = {}
    for kind, cnt in per_kind.items():
        if any(t_us[s] is None for s in cnt):
            continue
        blas_ms = sum(t_us[s] * c for s, c in cnt.items()) / steps * 1e-3
        rows = []
        for (kd, sh), (secs, n) in ours.items():
            if kd == kind:
                rows.append({"m_n_k": list(sh[:3]), "a_kmajor": sh[3], "b_kmajor": sh[4], "launches_per_step": n // steps, "us": round(secs / n * 1e6, 1),
                             "hipblaslt_us": round(t_us[sh], 1), "vs_hipblaslt": round(t_us[sh] / (secs / n * 1e6), 3)})
        rows.sort(key=lambda r: -r["us"] * r["launches_per_step"])
        out[names[kind]] = {"hipblaslt_ms_per_step": round(blas_ms, 3), "vs_hipblaslt": round(blas_ms / (ours_kind[kind] / steps * 1e3), 3), "shapes": rows[:8]}
    return out


HBM_KERNEL_FAMILIES = ("ln_fwd_kernel", "ln_bwd_kernel", "adamw_kernel", "sqnorm_kernel", "attn_fwd_mfma", "attn_bwd_", "row_copy_multi_kernel", "cast_kernel",
                       "splitk_reduce_kernel", "sparse_dwconv", "mse_", "patch_")


def hbm_kernel_rows(rel: str) -> dict | None:
    """The bandwidth side of the step (north_star: "rocprof HBM GB/s against chip peak"): for the LayerNorm / AdamW / attention / mover kernels, PMC HBM bytes per
    launch (FETCH_SIZE / WRITE_SIZE passes, gfx950-corrected) over the kernel's average duration in the rocprofv3 kernel summary OF THE SAME capture
    (tools/gpu_pmc_round.sh stores both in the stamped file) = achieved GB/s and its fraction of 8 TB/s.  Read from the committed file, not collected live."""
    try:
        meta = json.loads((ROOT / rel).read_text())
    except (OSError, ValueError):
        return None
    rows = {}
    for name, v in meta.get("kernels", {}).items():
        if v.get("avg_us") and name.startswith(HBM_KERNEL_FAMILIES):
            gbs = v["hbm_bytes_per_launch"] / (v["avg_us"] * 1e-6) / 1e9
            rows[name] = {"hbm_mb_per_launch": round(v["hbm_bytes_per_launch"] / 1e6, 1), "avg_us": v["avg_us"], "gb_s": round(gbs), "frac_of_8tb_s": round(gbs / HBM_PEAK_GBS, 3),
                          "ms_per_step": v.get("ms_per_step")}
    rows = dict(sorted(rows.items(), key=lambda kv: -(kv[1]["ms_per_step"] or 0.0))[:24])
    return {"kernels": rows, "source": f"committed {rel}: PMC bytes per launch / average duration of the kernel in the --kernel-trace summary of the same capture (one stream)",
            "stale": pmc_binding(rel)["stale"], "peak_gb_s": HBM_PEAK_GBS} if rows else None


def base_kwargs(size: str = "base", sax=(192, 192, 16), lax=(192, 192)) -> dict:  # noqa: ANN001
    from cinema_amd.vit import get_vit_config

    views = ["sax", "lax_2c", "lax_3c", "lax_4c"]
    return dict(image_size_dict={v: tuple(sax) if v == "sax" else tuple(lax) for v in views}, in_chans_dict=dict.fromkeys(views, 1),
                enc_patch_size_dict={v: (4, 4, 1) if v == "sax" else (4, 4) for v in views},
                enc_scale_factor_dict={v: (2, 2, 1) if v == "sax" else (2, 2) for v in views}, enc_conv_chans=[64, 128], enc_conv_n_blocks=2,
                **get_vit_config(size))


def synthetic_batch(kw: dict, batch: int, seed: int, device: str) -> dict:
    gen = torch.Generator().manual_seed(seed)
    return {v: torch.rand(batch, 1, *s, generator=gen).to(device) for v, s in kw["image_size_dict"].items()}


def cpu_baseline(kw: dict, state_dict: dict, batch: int, budget_s: float, device: str) -> tuple:
    """The CPU oracle (fp32, torch CPU ops on the host cores) on a bounded sample of the same workload -> (cpu_baseline, parity).
    ``parity``: the first step of the HIP path against the oracle on identical weights, inputs and masks (oracle/parity.py, checker only)."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import cinema_oracle as O  # noqa: N812
    from parity import mae_step_parity

    # intra-op threads actually used: torch's CPU kernels on this graph peak at ~16 threads on the 256-core GPU-box host
    # (probe run once with this function at different thread counts: 16 threads 3.6 s/step, 32 -> 4.2 s, 64 -> 7.6 s, 256 -> 640 s at batch 2)
    host_cores = os.cpu_count() or 1
    cores = min(host_cores, 16)
    torch.set_num_threads(cores)
    par = mae_step_parity(kw, state_dict, batch=batch, seed=7, device=device)
    parity = {"loss_rel": round(par["loss_rel"], 6), "grad_rel": round(par["grad_rel"], 5), "grad_norm_rel": round(par["grad_norm_rel"], 6),
              "worst_grad_rel_l2": {"name": par["worst_grad_rel_l2"]["name"], "value": round(par["worst_grad_rel_l2"]["value"], 5)},
              "view_loss_rel": {k: round(v, 6) for k, v in par["view_loss_rel"].items()}, "pred_max_abs": round(par["pred_max_abs"], 5),
              "loss": round(par["loss"], 6), "oracle_loss": round(par["oracle_loss"], 6),
              "what": f"first forward+backward of the HIP path vs the fp32 CPU oracle on identical weights, inputs and masks at batch {batch} of this workload; "
                      "grad_rel = worst relative L2 error over 10 named gradients (oracle/parity.py), worst_grad_rel_l2 over ALL parameters"}
    cfg = O.MAEConfig(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in kw.items()})
    trainer = O.Trainer({k: v.detach().float().cpu() for k, v in state_dict.items()}, cfg, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, clip_grad=5.0)
    gen = torch.Generator().manual_seed(99)
    images = {v: torch.rand(batch, 1, *s, generator=gen) for v, s in kw["image_size_dict"].items()}
    import math

    def masks() -> dict:
        return {v: O.random_patch_mask(batch, math.prod(cfg.grid_size(v)), 0.75, gen) for v in images}

    t0 = time.perf_counter()
    trainer.step(images, masks())  # warm-up (allocator, thread pool)
    warm = time.perf_counter() - t0
    n, t0 = 0, time.perf_counter()
    while n < 1 or (time.perf_counter() - t0 < budget_s and n < 8):
        loss, _, _, _ = trainer.step(images, masks())
        n += 1
    dt = time.perf_counter() - t0
    # SURVEY 8d asks for os.cpu_count() threads.  On the 256-core GPU-box host that setting is not measurable inside a bench run (one probe step at batch 2
    # took 640 s = 0.003 samples/s, torch's CPU kernels oversubscribe on this graph), so the line reports the fastest setting as `value` (16 threads), ONE live
    # step at 64 threads beside it (the trend), and the all-cores probe figure with its provenance.
    more = {}
    if host_cores >= 64 and budget_s >= 10:
        torch.set_num_threads(64)
        t1 = time.perf_counter()
        trainer.step(images, masks())
        more["64"] = round(batch / (time.perf_counter() - t1), 4)
        torch.set_num_threads(cores)
    all_cores = {"cores": host_cores, "value": 0.0031 if host_cores >= 128 else None,
                 "source": "probe at os.cpu_count() = 256 threads, one step at batch 2: 640 s (round 4, same host type); not re-timed in the default run"}
    return {"value": round(batch * n / dt, 4), "unit": "samples/s", "cores": cores, "host_cores": host_cores, "kind": "port", "samples_per_s_by_threads": {str(cores): round(batch * n / dt, 4), **more},
            "at_os_cpu_count_threads": all_cores,
            "sample": f"{n} optimisation steps (fwd+bwd+clip+AdamW) of the same Base 4-view config at batch {batch}, fp32 torch-CPU oracle, "
                      f"after 1 warm-up step ({warm:.1f} s); final loss {float(loss):.4f} (different data and step count than the GPU run: not comparable; "
                      f"see `parity` for the like-for-like comparison); {cores} intra-op threads of the host's {host_cores} cores (more threads are slower on this graph)"}, parity


DUMP_PARAM_SAMPLE = 1 << 22  # updated weights written by --dump-outputs: 4 Mi fp32 values (16 MB)


def dump_outputs(out_dir: str, loss: torch.Tensor, grad_norm: torch.Tensor, metrics: dict, model: torch.nn.Module) -> None:
    """``--dump-outputs``: what a caller of the timed step received from its last call, as float32 ``<name>.npy`` files - ``loss``, ``grad_norm``, one
    ``metric_<key>`` per metric tensor, and ``params_sample``, the weights after that step's update: all parameters concatenated in ``named_parameters``
    order (the reference's state_dict order), or a fixed-seed sample of DUMP_PARAM_SAMPLE of them (sorted positions) when there are more."""
    import numpy as np

    arrays = {"loss": loss, "grad_norm": grad_norm, **{f"metric_{k}": v for k, v in metrics.items()}}
    arrays = {k: torch.as_tensor(v).detach().float().cpu().numpy() for k, v in arrays.items()}
    with torch.no_grad():
        flat = torch.cat([p.detach().reshape(-1).float() for _, p in model.named_parameters()])
        if flat.numel() > DUMP_PARAM_SAMPLE:
            pos = torch.randint(0, flat.numel(), (DUMP_PARAM_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
            flat = flat[pos.to(flat.device)]
        arrays["params_sample"] = flat.cpu().numpy()
    path = Path(out_dir)
    path.mkdir(parents=True, exist_ok=True)
    for name, arr in arrays.items():
        np.save(path / f"{name}.npy", arr)


def result_line(out: dict) -> dict:
    """The printed result line: ``out`` without the per-kernel tables of ``roofline`` and with ``secondary`` cut to each configuration's step time.  The whole
    object (over 8 KB at the default workload) no longer fits in what a driver keeps of a run's output; ``--details FILE`` writes all of it."""
    line = dict(out)
    if isinstance(line.get("roofline"), dict):
        line["roofline"] = {k: v for k, v in line["roofline"].items() if k not in ("all_gemm_kernels", "hbm_kernels", "traffic_binding")}
    if isinstance(line.get("secondary"), dict):
        line["secondary"] = {k: ({m: v[m] for m in ("ms_per_step", "samples_per_s", "error") if m in v} if isinstance(v, dict) else v)
                             for k, v in line["secondary"].items()}
    return line


def emit(out: dict, details: str | None) -> None:
    if details:
        Path(details).write_text(json.dumps(out) + "\n")
    print(json.dumps(result_line(out)), flush=True)


def _latest_profile(suffix: str) -> str:
    """Newest committed counter capture by round prefix (profiles/rNN_<suffix>; tools/gpu_pmc_round.sh writes them, stamped with the library's sha256)."""
    hits = sorted(p.name for p in (ROOT / "profiles").glob(f"r[0-9][0-9]_{suffix}"))
    return f"profiles/{hits[-1]}" if hits else f"profiles/{suffix}"


PMC_TRAFFIC_FILE = _latest_profile("pmc_hbm_traffic.json")
PMC_MFMA_FILE = _latest_profile("mfma_util.json")
PMC_TRAFFIC_FP8_FILE = _latest_profile("pmc_hbm_traffic_fp8.json")


def _committed(rel: str, kernel: str):  # noqa: ANN202
    try:
        return json.loads((ROOT / rel).read_text())["kernels"].get(kernel)
    except (OSError, ValueError, KeyError):
        return None


def pmc_binding(rel: str) -> dict:
    """Ties a committed counter file to the binary that is being timed: the file carries the sha256 of the library its passes ran
    (tools/gpu_pmc_round.sh); ``stale`` says whether that is NOT the library loaded by this process."""
    import hashlib

    from cinema_amd import hip as K

    try:
        meta = json.loads((ROOT / rel).read_text())
    except (OSError, ValueError):
        return {"file": rel, "stale": None}
    loaded = hashlib.sha256(Path(K.library_path()).read_bytes()).hexdigest()
    return {"file": rel, "so_sha256": meta.get("so_sha256"), "git_head": meta.get("git_head"), "loaded_so_sha256": loaded,
            "stale": meta.get("so_sha256") != loaded}


def pmc_traffic(kernel: str):  # noqa: ANN201
    """HBM bytes per launch of ``kernel`` from the COMMITTED rocprofv3 PMC passes of this same command (tools/gpu_pmc_bench.sh ->
    profiles/pmc_hbm_traffic.json; FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md); None when no capture is committed.
    Not a live measurement: counter collection needs rocprofv3 around the process."""
    hit = _committed(PMC_TRAFFIC_FILE, kernel)
    return None if hit is None else hit["hbm_bytes_per_launch"]


def pmc_mfma_util(kernel: str):  # noqa: ANN201
    """SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs) of ``kernel`` from the committed PMC passes (tools/gpu_pmc_mfma.sh)."""
    hit = _committed(PMC_MFMA_FILE, kernel)
    return None if hit is None else hit.get("mfma_util")


SEG_STEP_GFLOP_PER_SAMPLE = 3 * 1412.9  # BASELINE.md section 2, config 4 (ConvUNetR Base, SAX 256x256x12): 3 x forward of the reference graph


def seg_kwargs(size: str = "base", sax=(256, 256, 12)) -> dict:  # noqa: ANN001
    """ConvUNetR of the ACDC recipe (cinema/segmentation/acdc/config.yaml:52-65) at the BASELINE config-4 input size."""
    from cinema_amd.vit import get_vit_config

    vit = get_vit_config(size)
    return dict(image_size_dict={"sax": tuple(sax)}, in_chans_dict={"sax": 1}, out_chans=4, enc_patch_size_dict={"sax": (4, 4, 1)},
                enc_scale_factor_dict={"sax": (2, 2, 1)}, enc_conv_chans=[64, 128], enc_conv_n_blocks=2, enc_embed_dim=vit["enc_embed_dim"],
                enc_depth=vit["enc_depth"], enc_n_heads=vit["enc_n_heads"], dec_chans=(32, 64, 128, 256, 512), dec_patch_size_dict={"sax": (2, 2, 1)},
                dec_scale_factor_dict={"sax": (2, 2, 1)}, dropout=0.1, drop_path=0.1)


def seg_cpu_baseline(kw: dict, state_dict: dict, device: str, budget_s: float) -> tuple:
    """(cpu_baseline, parity) for the segmentation task: the fp32 CPU oracle's ConvUNetR forward + loss + backward on ONE sample of the same
    shape (the sample of the baseline), and - the config-4 acceptance - the HIP path against the oracle on that sample (oracle/parity.py,
    checker only): argmax agreement, the Dice of the two argmax segmentations, loss and gradient-norm errors."""
    sys.path.insert(0, str(ROOT / "oracle"))
    from parity import seg_step_parity

    host_cores = os.cpu_count() or 1
    cores = min(host_cores, 16)
    par = seg_step_parity(kw, state_dict, device=device, threads=cores)
    dt = par["oracle_seconds"]
    parity = {"argmax_agreement": round(par["argmax_agreement"], 5), "dice_gpu_vs_cpu_segmentation": round(par["dice_gpu_vs_cpu_segmentation"], 5),
              "logits_max_abs": round(par["logits_max_abs"], 4), "logits_abs_max_ref": round(par["logits_abs_max_ref"], 3),
              "loss_rel": round(par["loss_rel"], 6), "grad_norm_rel": round(par["grad_norm_rel"], 5),
              "worst_grad_rel_l2": {"name": par["worst_grad_rel_l2"]["name"], "value": round(par["worst_grad_rel_l2"]["value"], 4)},
              "worst_grad_err_over_global_norm": {"name": par["worst_grad_err_over_global_norm"]["name"], "value": round(par["worst_grad_err_over_global_norm"]["value"], 6)},
              "what": "HIP path (dropout / drop_path off) vs the fp32 CPU oracle on one identical sample and identical weights (random init): fraction of voxels "
                      "with the same argmax class and the foreground Dice between the two argmax segmentations of the eval-mode logits (acceptance: >= 0.995, "
                      "|1 - Dice| <= 0.01); CE + Dice loss, global gradient norm and worst per-tensor gradient of the training-mode step"}
    del budget_s
    return {"value": round(1.0 / dt, 4), "unit": "samples/s", "cores": cores, "host_cores": host_cores, "kind": "port",
            "sample": f"1 forward + CE/Dice loss + backward of the same ConvUNetR config at batch 1 (fp32 torch-CPU oracle, no optimiser update), {dt:.1f} s, "
                      f"{cores} intra-op threads of the host's {host_cores} cores"}, parity


def seg_main(args, rank: int, world: int, device: str, sync) -> None:  # noqa: ANN001
    """BASELINE config 4: ConvUNetR fine-tuning step (forward, CE + Dice, backward, [gradient all-reduce], clip 5, layer-decay AdamW) on synthetic
    SAX volumes resident in HBM; dropout / drop_path 0.1 as in the reference recipe; weak scaling, whole-job samples/s."""
    import torch.distributed as dist

    from cinema_amd import hip as K
    from cinema_amd.segmentation.convunetr import ConvUNetR
    from cinema_amd.segmentation.train import SegTrainStep

    batch_size = args.batch if args.batch != 16 else 4  # reference batch_size_per_device (acdc/config.yaml:42); --batch overrides
    sax = tuple(int(v) for v in args.sax.split(",")) if args.sax != "192,192,16" else (256, 256, 12)
    kw = seg_kwargs(args.size, sax)
    torch.manual_seed(0)
    model = ConvUNetR(**kw)
    cpu_state = {k: v.detach().clone() for k, v in model.state_dict().items()} if rank == 0 else None
    model.to(device).train()
    step = SegTrainStep(model, ["sax"], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, layer_decay=0.75, clip_grad=5.0, synchronizer=sync, replay=not args.eager)
    gen = torch.Generator().manual_seed(1234 + rank)
    batches = []
    for _ in range(2):
        image = torch.rand(batch_size, 1, *sax, generator=gen)
        batches.append({"sax_image": image.to(device), "sax_label": torch.clamp((image * 4).long(), 0, 3).to(torch.int8).to(device)})

    def barrier() -> None:
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    extra_untimed = max(0, min(args.prewarm, 5) - args.warmup)
    for i in range(extra_untimed + args.warmup):
        loss, gnorm, _ = step(batches[i % 2])
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss, gnorm, metrics = step(batches[i % 2])
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    final_loss = float(loss)
    peak_gib = round(torch.cuda.max_memory_reserved() / 2**30, 1)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, gnorm, metrics, model)
    n_launches = next(iter(step._recorded.values())).n_launches if step._recorded else None  # noqa: SLF001
    step.replay = False  # the per-launch event timing below goes through the module code
    roofline = None
    if args.profile_steps > 0:
        from cinema_amd import tape as T_

        side, T_.SIDE_WGRAD = T_.SIDE_WGRAD, False
        step(batches[0])
        if rank == 0:
            K.GEMM_PROFILE = []
        for i in range(args.profile_steps):
            step(batches[i % 2])
        barrier()
        prof, K.GEMM_PROFILE = K.GEMM_PROFILE, None
        T_.SIDE_WGRAD = side
        if rank == 0:
            agg: dict = {}
            for kind, flops, e0, e1, _shape, *_ in prof:
                a = agg.setdefault(kind, [0.0, 0.0, 0])
                a[0] += flops
                a[1] += e0.elapsed_time(e1) * 1e-3
                a[2] += 1
            kind = max(agg, key=lambda k: agg[k][1])
            flops, secs, n = agg[kind]
            achieved = flops / secs / 1e12
            roofline = {"bound": "mfma",  # (the implicit-convolution launches carry no algorithmic byte count: priced against the MFMA peak) "kernel": K.GEMM_KERNEL_NAMES[kind], "achieved": round(achieved, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None, "launches_per_step": n // args.profile_steps,
                        "avg_launch_us": round(secs / n * 1e6, 2), "gflop_per_launch": round(flops / n / 1e9, 3),
                        "timing": "HIP events on the launch stream around every launch of this kernel, live in this process",
                        "gemm_ms_per_step": round(sum(v[1] for v in agg.values()) / args.profile_steps * 1e3, 2),
                        "all_gemm_kernels": {K.GEMM_KERNEL_NAMES[k]: {"tflops": round(v[0] / v[1] / 1e12, 1), "ms_per_step": round(v[1] / args.profile_steps * 1e3, 3),
                                                                      "launches_per_step": v[2] // args.profile_steps} for k, v in agg.items()}}
    if rank == 0:
        samples_per_s = world * batch_size * args.steps / dt
        out = {"metric": "ConvUNetR segmentation fine-tune samples/sec (SAX 256x256x12, 4 classes; BASELINE config 4)", "value": round(samples_per_s, 2),
               "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "untimed_steps": extra_untimed + args.warmup,
               "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": f"ConvUNetR ViT-{args.size.capitalize()} (ACDC decoder recipe), SAX {'x'.join(str(v) for v in sax)}, 4 classes, per-GPU batch "
                                      f"{batch_size}, dropout 0.1 / drop_path 0.1, fwd + CE/Dice + bwd + clip(5.0) + layer-decay(0.75) AdamW, random-init weights",
                          "global_batch": world * batch_size, "parallelism": f"dp{world}", "final_loss": round(final_loss, 5), "peak_mem_gib": peak_gib,
                          "host": ("module code issues every launch (--eager)" if args.eager else
                                   f"forward + loss + backward re-issued from a recorded list of {n_launches} HIP launches (cinema_amd/replay.py); clip+AdamW eager"),
                          "reference_equiv_tflops_per_gpu": round(samples_per_s / world * SEG_STEP_GFLOP_PER_SAMPLE / 1e3, 1) if sax == (256, 256, 12) and args.size == "base" else None},
               "roofline": roofline}
        if world == 1 and args.cpu_budget > 0:
            out["cpu_baseline"], out["parity"] = seg_cpu_baseline(kw, cpu_state, device, args.cpu_budget)
        emit(out, args.details)


def secondary_configs(device: str, with_parity: bool) -> dict:
    """BASELINE configs 4 and 5 in the same process, short (a few seconds of GPU time each), so that the driver's one run times them too:
    config4 = ConvUNetR fine-tuning step (SAX 256x256x12, batch 4, recorded step); config5_fp8 = ViT-Large MAE step at 256x256x24 + 3 LAX 256x256,
    batch 8, e4m3 forward projections, with the bf16 time of the same shape beside it.  Parity objects from oracle/parity.py (checker only)."""
    import gc

    from cinema_amd import CineMA
    from cinema_amd import tape as T_
    from cinema_amd.optim import TrainStep
    from cinema_amd.segmentation.convunetr import ConvUNetR
    from cinema_amd.segmentation.train import SegTrainStep

    sys.path.insert(0, str(ROOT / "oracle"))
    out: dict = {}

    def timed(fn, warm: int, n: int) -> float:  # noqa: ANN001
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    # ---- config 4
    kw = seg_kwargs("base", (256, 256, 12))
    torch.manual_seed(0)
    model = ConvUNetR(**kw)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(device).train()
    step = SegTrainStep(model, ["sax"], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, layer_decay=0.75, clip_grad=5.0, replay=True)
    gen = torch.Generator().manual_seed(1234)
    image = torch.rand(4, 1, 256, 256, 12, generator=gen)
    batch = {"sax_image": image.to(device), "sax_label": torch.clamp((image * 4).long(), 0, 3).to(torch.int8).to(device)}
    ms = timed(lambda: step(batch), 6, 12)
    out["config4"] = {"workload": "ConvUNetR ViT-Base (ACDC decoder recipe), SAX 256x256x12, 4 classes, per-GPU batch 4, dropout / drop_path 0.1, fwd + CE/Dice + bwd + "
                                  "clip + layer-decay AdamW, recorded step", "ms_per_step": round(ms, 3), "samples_per_s": round(4e3 / ms, 2), "steps": 12, "warmup": 6,
                      "dtype": "bf16", "reference_equiv_tflops_per_gpu": round(4e3 / ms * SEG_STEP_GFLOP_PER_SAMPLE / 1e3, 1)}
    del step, model
    gc.collect()
    torch.cuda.empty_cache()
    if with_parity:
        from parity import seg_step_parity

        par = seg_step_parity(kw, sd, device=device, threads=min(os.cpu_count() or 1, 16))
        out["config4"]["parity"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in par.items()}
        out["config4"]["parity"]["what"] = "HIP path vs fp32 CPU oracle, one identical sample: argmax agreement / Dice of the argmax segmentations (>= 0.995, |1 - Dice| <= 0.01), loss and gradients"
    # ---- config 2 at the reference's GLOBAL batch: the recipe is 64 samples per optimiser step = 16 per device x world x accumulation (mae/config.yaml:44-45,
    # pretrain.py:259-269), i.e. four accumulated micro-steps of 16 on one GPU; 288 GB hold the 64 in ONE micro-step, which is the same update
    kw2 = base_kwargs("base")
    torch.manual_seed(0)
    model = CineMA(**kw2).to(device)
    st = TrainStep(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, clip_grad=5.0, replay=True)
    b64 = synthetic_batch(kw2, 64, 1234, device)
    ms = timed(lambda: st(b64, 0.75), 4, 8)
    out["config2_global_batch_64"] = {"workload": "CineMA ViT-Base MAE, 4 views, mask 0.75, bf16, ONE micro-step of 64 samples on one GPU (the reference's optimiser step at global batch "
                                                  "64; the headline keeps its per-device 16)", "ms_per_step": round(ms, 3), "samples_per_s": round(64e3 / ms, 2), "steps": 8, "warmup": 4,
                                      "reference_equiv_tflops_per_gpu": round(64e3 / ms * STEP_GFLOP_PER_SAMPLE / 1e3, 1)}
    del st, model, b64
    gc.collect()
    torch.cuda.empty_cache()
    # ---- config 5 shape: bf16 and fp8 forward
    kw5 = base_kwargs("large", (256, 256, 24), (256, 256))
    torch.manual_seed(0)
    model = CineMA(**kw5)
    sd5 = {k: v.detach().clone() for k, v in model.state_dict().items()} if with_parity else None
    model.to(device)
    b5 = synthetic_batch(kw5, 8, 4321, device)
    res = {}
    fp8_roof = None
    prev = T_.FP8_FORWARD
    try:
        for name, fp8 in (("bf16", False), ("fp8", True)):
            T_.FP8_FORWARD = fp8
            st = TrainStep(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, clip_grad=5.0, replay=True)
            res[name] = timed(lambda: st(b5, 0.75), 4, 6)  # noqa: B023  (fp8: the first warm-up step records the maxima of the delayed scales, eager)
            if fp8:  # roofline of the e4m3 weight-gradient kernel: HIP events around every launch of two eager steps, against the 5 PF dense fp8 peak
                from cinema_amd import hip as K_

                st.replay = False
                K_.GEMM_PROFILE = []
                side_prev, T_.SIDE_WGRAD = T_.SIDE_WGRAD, False
                try:
                    for _ in range(2):
                        st(b5, 0.75)
                    torch.cuda.synchronize()
                    recs = [r for r in K_.GEMM_PROFILE if r[0] == 4096 + 3 + 8 * 4]
                finally:
                    K_.GEMM_PROFILE = None
                    T_.SIDE_WGRAD = side_prev
                if recs:
                    secs = sum(r[2].elapsed_time(r[3]) for r in recs) * 1e-3
                    flops = sum(r[1] for r in recs)
                    alg = sum(r[4][6] for r in recs)
                    fp8_roof = {"bound": "mfma", "kernel": K_.GEMM_KERNEL_NAMES[4096 + 3 + 8 * 4], "achieved": round(flops / secs / 1e12, 1), "peak": 5000.0, "unit": "TFLOP/s",
                                "frac": round(flops / secs / 5e15, 4), "intensity_flop_per_byte": round(flops / max(alg, 1.0), 1), "ridge_flop_per_byte": 625.0,
                                "launches_per_step": len(recs) // 2, "avg_launch_us": round(secs / len(recs) * 1e6, 2),
                                "gflop_per_launch": round(flops / len(recs) / 1e9, 3), "algorithmic_bytes_per_launch": int(alg / len(recs)),
                                "traffic": (_committed(PMC_TRAFFIC_FP8_FILE, K_.GEMM_KERNEL_NAMES[4096 + 3 + 8 * 4]) or {}).get("hbm_bytes_per_launch"),
                                "traffic_source": f"committed {PMC_TRAFFIC_FP8_FILE} (FETCH_SIZE / WRITE_SIZE passes over this config's fp8 step, tools/gpu_r06_final.sh)",
                                "traffic_stale": pmc_binding(PMC_TRAFFIC_FP8_FILE)["stale"],
                                "timing": "HIP events on the launch stream around every launch (two eager steps, one stream)",
                                "what": "weight gradients of a transformer block (qkv, proj, fc1, fc2) on row-major e4m3 operands in one persistent launch, k-slices reduced in the launch"}
            del st
            gc.collect()
    finally:
        T_.FP8_FORWARD = prev
    out["config5_fp8"] = {"workload": "CineMA ViT-Large MAE, 4 views (SAX 256x256x24 + 3 LAX 256x256), mask 0.75, per-GPU batch 8, fwd+bwd+clip+AdamW, recorded step",
                          "dtype": "fp8 (OCP e4m3 on the MX-scaled MFMA for the forward projections, data gradients AND weight gradients of the transformer blocks; weights: "
                                   "per-tensor current scaling; activations / gradients: per-tensor DELAYED scaling, 8-bit copies written by the producing kernels; "
                                   "attention, LayerNorm, loss, optimiser in bf16 / fp32)", "ms_per_step": round(res["fp8"], 3),
                          "samples_per_s": round(8e3 / res["fp8"], 2), "bf16_ms_per_step": round(res["bf16"], 3), "fp8_speedup_over_bf16": round(res["bf16"] / res["fp8"], 4),
                          "steps": 6, "warmup": 4, "reference_equiv_tflops_per_gpu": round(8e3 / res["fp8"] * 3 * 1806.7 / 1e3, 1), "roofline": fp8_roof}
    del model
    gc.collect()
    torch.cuda.empty_cache()
    if with_parity:
        from parity import mae_loss_parity

        par = mae_loss_parity(kw5, sd5, batch=1, device=device, fp8=True, threads=min(os.cpu_count() or 1, 16))
        out["config5_fp8"]["parity"] = {"loss_rel": round(par["loss_rel"], 6), "loss": round(par["loss"], 6), "oracle_loss": round(par["oracle_loss"], 6),
                                        "view_loss_rel": {k: round(v, 6) for k, v in par["view_loss_rel"].items()},
                                        "what": "first-step loss (forward) of the fp8 path vs the fp32 CPU oracle at this shape, batch 1, identical weights / inputs / masks (stated: <= 5e-2)"}
        # ... and the GRADIENTS at this very shape (the oracle's forward + backward takes ~13 s of host time): whole gradient, worst matrix, six named tensors, bf16 and e4m3
        from parity import mae_fp8_grad_parity as _gp5

        names5 = ("encoder.blocks.0.attn.kv.weight", "encoder.blocks.23.mlp.fc1.weight", "decoder.blocks.0.attn.q.weight", "decoder.blocks.7.mlp.fc2.weight",
                  "enc_down_dict.sax.conv_blocks.0.conv.0.mlp.fc1.weight", "pred_head_dict.sax.weight")
        g5 = _gp5(kw5, sd5, batch=1, seed=17, device=device, threads=min(os.cpu_count() or 1, 16), modes=("bf16", "fp8_wgrad"), report=names5)
        out["config5_fp8"]["parity"]["gradients_own_shape"] = {
            m: {"loss_rel": round(g5[m]["loss_rel"], 6), "grad_norm_rel": round(g5[m]["grad_norm_rel"], 6), "whole_grad_rel_l2": round(g5[m]["whole_grad_rel_l2"], 5),
                "worst_matrix_rel_l2": {"name": g5[m]["worst_matrix_rel_l2"]["name"], "value": round(g5[m]["worst_matrix_rel_l2"]["value"], 5)},
                "named_rel_l2": g5[m]["named_rel_l2"]} for m in ("bf16", "fp8_wgrad")}
        out["config5_fp8"]["parity"]["gradients_own_shape"]["what"] = ("gradients of the HIP path vs the fp32 CPU oracle at config 5's own spatial size and depth, batch 1, identical weights / "
                                                                       f"inputs / masks (oracle forward + backward {g5['oracle_seconds']} s): bf16 path and the full e4m3 path")
        # gradients of the fp8 path against the ORACLE (its backward at the config-5 shape takes minutes: a 2 + 2 block model with MFMA-sized channels instead)
        from parity import mae_fp8_grad_parity

        views = ["sax", "lax_2c"]
        kwm = dict(image_size_dict={"sax": (64, 64, 8), "lax_2c": (64, 64)}, in_chans_dict=dict.fromkeys(views, 1), enc_patch_size_dict={"sax": (4, 4, 1), "lax_2c": (4, 4)},
                   enc_scale_factor_dict={"sax": (2, 2, 1), "lax_2c": (2, 2)}, enc_conv_chans=[64, 128], enc_conv_n_blocks=1, enc_embed_dim=256, enc_depth=2, enc_n_heads=4,
                   dec_embed_dim=128, dec_depth=2, dec_n_heads=4)
        torch.manual_seed(3)
        sdm = {k: v.detach().clone() for k, v in CineMA(**kwm).state_dict().items()}
        gp = mae_fp8_grad_parity(kwm, sdm, batch=3, seed=5, device=device, threads=min(os.cpu_count() or 1, 16))
        out["config5_fp8"]["parity"]["gradients_midsize"] = {
            m: {"loss_rel": round(gp[m]["loss_rel"], 6), "grad_norm_rel": round(gp[m]["grad_norm_rel"], 6), "whole_grad_rel_l2": round(gp[m]["whole_grad_rel_l2"], 5),
                "worst_matrix_rel_l2": round(gp[m]["worst_matrix_rel_l2"]["value"], 5), "worst_vector_rel_l2": round(gp[m]["worst_vector_rel_l2"]["value"], 5),
                "fp8_dgrad_gemms": gp[m]["fp8_dgrad_gemms"], "fp8_wgrad_problems": gp[m]["fp8_wgrad_problems"]} for m in ("bf16", "fp8_wgrad")}
        # ... and at config 5's FULL depth (ViT-Large 24 + 8 blocks) on a small spatial size, where the oracle's backward takes seconds
        from cinema_amd.vit import get_vit_config

        kwd = dict(image_size_dict={"sax": (96, 96, 8), "lax_2c": (96, 96)}, in_chans_dict=dict.fromkeys(views, 1), enc_patch_size_dict={"sax": (4, 4, 1), "lax_2c": (4, 4)},
                   enc_scale_factor_dict={"sax": (2, 2, 1), "lax_2c": (2, 2)}, enc_conv_chans=[64, 128], enc_conv_n_blocks=2, **get_vit_config("large"))
        torch.manual_seed(11)
        sdd = {k: v.detach().clone() for k, v in CineMA(**kwd).state_dict().items()}
        gd = mae_fp8_grad_parity(kwd, sdd, batch=2, seed=13, device=device, threads=min(os.cpu_count() or 1, 16), modes=("bf16", "fp8_wgrad"))
        out["config5_fp8"]["parity"]["gradients_full_depth"] = {
            m: {"loss_rel": round(gd[m]["loss_rel"], 6), "grad_norm_rel": round(gd[m]["grad_norm_rel"], 6), "whole_grad_rel_l2": round(gd[m]["whole_grad_rel_l2"], 5),
                "worst_matrix_rel_l2": {"name": gd[m]["worst_matrix_rel_l2"]["name"], "value": round(gd[m]["worst_matrix_rel_l2"]["value"], 5)},
                "worst_vector_rel_l2": {"name": gd[m]["worst_vector_rel_l2"]["name"], "value": round(gd[m]["worst_vector_rel_l2"]["value"], 5)},
                "block_matrix_rel_l2_first_last": {b: gd[m]["block_matrix_rel_l2"].get(b) for b in ("encoder.00", "encoder.23", "decoder.00", "decoder.07")},
                "fp8_dgrad_gemms": gd[m]["fp8_dgrad_gemms"], "fp8_wgrad_problems": gd[m]["fp8_wgrad_problems"]} for m in ("bf16", "fp8_wgrad")}
        out["config5_fp8"]["parity"]["gradients_full_depth"]["what"] = ("the same comparison on a model with config 5's full depth and widths (ViT-Large: 24 + 8 blocks, 1024 / 512 channels) at "
                                                                         "SAX 96x96x8 + one long-axis view 96x96, batch 2 (the oracle's backward at the config-5 spatial size takes minutes); "
                                                                         "block_matrix_rel_l2: encoder block 0 / 23, decoder block 0 / 7")
        out["config5_fp8"]["parity"]["gradients_midsize"]["what"] = ("gradients of the HIP path vs the fp32 CPU oracle on a 2 + 2 block model (encoder 256, decoder 128 channels), batch 3, "
                                                                     "identical weights / inputs / masks: bf16 path and the full fp8 path (a first pass records the delayed scales)")
    return out


def self_launch(n_gpus: int) -> int:
    """``python bench.py --gpus N`` without a launcher: re-run this command line under ``torch.distributed.run`` with N ranks on this node (rendezvous on
    127.0.0.1, a free port) and hand back its exit code.  The children see WORLD_SIZE and take the ordinary path; their stdout (rank 0's one JSON line) and
    stderr are this process' own."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes fails without it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(Path(__file__).resolve()), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16, help="per-GPU batch (reference batch_size_per_device, mae/config.yaml:45)")
    ap.add_argument("--size", default="base")
    ap.add_argument("--sax", default="192,192,16", help="SAX volume size (BASELINE config 5: 256,256,24 with --size large --lax 256,256)")
    ap.add_argument("--lax", default="192,192", help="long-axis view size")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="seconds of CPU-oracle timing (0 disables)")
    ap.add_argument("--prewarm", type=int, default=20, help="untimed steps run in total before the timed region (>= --warmup); 0 for profiling runs")
    ap.add_argument("--force-sync", action="store_true", help="N=1 only: still issue the gradient collectives (RCCL path check)")
    ap.add_argument("--profile-steps", type=int, default=2, help="extra instrumented steps for the per-kernel roofline")
    ap.add_argument("--task", default="mae", choices=["mae", "seg"], help="mae: the BASELINE metric (config 2 / 3 / 5 shapes); seg: BASELINE config 4, the "
                    "ConvUNetR segmentation fine-tuning step (SAX 256x256x12, 4 classes, per-GPU batch 4, dropout / drop_path 0.1)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"], help="fp8: the transformer blocks' forward projections and data gradients on e4m3 operands (BASELINE config 5, "
                    "with --size large --sax 256,256,24 --lax 256,256 --batch 8); weight gradients stay bf16.  The BASELINE metric (config 2) is bf16")
    ap.add_argument("--eager", action="store_true", help="issue every launch from the module code instead of the recorded launch list (A/B)")
    ap.add_argument("--grad-exchange", default="fp32", choices=["fp32", "bf16"], help="dtype of the gradient all-reduce payload (N > 1): bf16 halves the xGMI bytes")
    ap.add_argument("--exchange", default=os.environ.get("CINEMA_GRAD_EXCHANGE", "all_reduce"), choices=["all_reduce", "rs_ag"],
                    help="gradient exchange algorithm (N > 1): all_reduce = torch.distributed.all_reduce per range (RCCL chooses ring / tree / direct); rs_ag = explicit "
                         "reduce_scatter_tensor + all_gather_into_tensor on the flat ranges (one-hop phases on the fully connected xGMI mesh)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short config-4 / config-5 measurements appended to the default one-GPU line")
    ap.add_argument("--no-blas-reference", action="store_true", help="skip the hipBLASLt timing of the step's GEMM shapes (roofline.all_gemm_kernels[*].vs_hipblaslt)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned (loss, gradient norm, metrics, a fixed sample of the updated "
                    "weights) as float32 DIR/<name>.npy; the inputs depend on the arguments only, so two builds can be compared output for output")
    ap.add_argument("--details", metavar="FILE", help="write the whole result object (per-kernel tables, secondary configurations with their parity) to FILE; "
                    "the printed line leaves those tables out")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N` (no launcher): become the launcher - one rank per GPU under torch.distributed.run, the same command line the
        # driver documents (reference: cinema/mae/pretrain.py:441-448 spawns its ranks itself); rank 0's JSON line is this process' stdout
        raise SystemExit(self_launch(args.gpus))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus} (or plain `python bench.py --gpus {args.gpus}`)")
    if not torch.cuda.is_available():
        raise SystemExit(f"bench.py needs an MI355X: the HIP path has no CPU fallback (rank {os.environ.get('RANK', '0')} of {world})")
    # path check of the multi-rank branch on a ONE-GPU box (dev only, never a metric): CINEMA_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and
    # CINEMA_BENCH_BACKEND=gloo replaces RCCL, which refuses two ranks on one device
    backend = os.environ.get("CINEMA_BENCH_BACKEND", "nccl")
    if os.environ.get("CINEMA_BENCH_SHARE_GPU") == "1":
        local_rank = 0
        # two processes x (main + weight-gradient + long-axis stream) oversubscribe the hardware queues of ONE device: the shared-GPU check took 162 s instead of
        # 9 s with the third stream (one process per GPU - the product layout - gains from it with RCCL collectives too: --force-sync 27.68 -> 27.38 ms)
        os.environ.setdefault("CINEMA_LAX_STREAM", "0")
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"

    import torch.distributed as dist

    from cinema_amd import CineMA
    from cinema_amd import hip as K
    from cinema_amd import tape as T_fp8
    from cinema_amd.ddp import GradientSynchronizer, ddp_setup
    from cinema_amd.optim import TrainStep

    T_fp8.FP8_FORWARD = args.dtype == "fp8"

    sync = None
    if world > 1:
        ddp_setup(rank, world, backend=backend)
        sync = GradientSynchronizer(world, exchange_dtype=torch.bfloat16 if args.grad_exchange == "bf16" else torch.float32, algorithm=args.exchange)
    elif args.force_sync:  # one-process RCCL group: runs the overlapped all-reduce schedule on one GPU (path check, not a metric)
        os.environ.setdefault("MASTER_PORT", "29533")
        ddp_setup(0, 1, backend="nccl")
        sync = GradientSynchronizer(1, force_collectives=True, exchange_dtype=torch.bfloat16 if args.grad_exchange == "bf16" else torch.float32, algorithm=args.exchange)

    if args.task == "seg":
        seg_main(args, rank, world, device, sync)
        if world > 1 or args.force_sync:
            dist.destroy_process_group()
        return

    kw = base_kwargs(args.size, tuple(int(v) for v in args.sax.split(",")), tuple(int(v) for v in args.lax.split(",")))
    torch.manual_seed(0)  # identical weights on every rank (config.seed, mae/config.yaml:1)
    model = CineMA(**kw)
    cpu_state = {k: v.detach().clone() for k, v in model.state_dict().items()} if rank == 0 else None
    model.to(device)
    step = TrainStep(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, clip_grad=5.0, synchronizer=sync, replay=not args.eager)
    torch.manual_seed(1234 + rank)  # per-rank mask / data streams (pretrain.py:309-310)
    batches = [synthetic_batch(kw, args.batch, 1234 + rank * 100 + i, device) for i in range(2)]

    def barrier() -> None:
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    loss = None
    # steady state needs ~20 steps (caching-allocator growth, clock ramp: 38.7 -> 36.0 ms/step measured between steps 10 and 50); when the
    # caller asks for fewer warm-up steps the difference is run here, untimed, before the W warm-up steps of the contract
    extra_untimed = max(0, args.prewarm - args.warmup)
    for i in range(extra_untimed):
        step(batches[i % 2], 0.75)
    for i in range(args.warmup):
        loss, gnorm, _ = step(batches[i % 2], 0.75)
    barrier()
    k0 = K.kernel_launch_count()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss, gnorm, metrics = step(batches[i % 2], 0.75)
    barrier()
    dt = time.perf_counter() - t0
    kernels_per_step = round((K.kernel_launch_count() - k0) / max(1, args.steps), 1)  # the library's own count over the timed steps (+ 1 torch fill: zero_grad)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    final_loss = float(loss)
    n_launches = next(iter(step._recorded.values())).n_launches if step._recorded else None  # noqa: SLF001
    peak_gib = round(torch.cuda.max_memory_reserved() / 2**30, 1)  # of 288: parameters + optimiser state + the recorded step's private pool
    if args.dump_outputs and rank == 0:  # before the information-only steps below overwrite the step's outputs and update the weights again
        dump_outputs(args.dump_outputs, loss, gnorm, metrics, model)
    # ---- N > 1: how much of the gradient exchange hides behind the backward pass (every rank runs the same extra steps; the replicas diverge
    # in the "no exchange" mode, which is why this comes after the timed region).  exposed = overlapped step - step without exchange;
    # unoverlapped = step with every collective after the backward - step without exchange
    ddp_info = None
    if world > 1 and sync is not None and args.profile_steps > 0:
        def mode_ms(n: int = 8) -> float:
            for i in range(2):
                step(batches[i % 2], 0.75)
            barrier()
            t0m = time.perf_counter()
            for i in range(n):
                step(batches[i % 2], 0.75)
            barrier()
            t = torch.tensor([time.perf_counter() - t0m], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t) / n * 1e3

        ranks = [None] * world
        dist.all_gather_object(ranks, (rank, torch.cuda.get_device_name(local_rank), local_rank))
        overlapped = mode_ms()
        payload_bytes, n_early, n_coll = sync.bytes_last, sync.n_early_last, sync.n_collectives_last  # of the overlapped schedule (the two measurement modes below change them)
        sync.defer_all = True
        at_end = mode_ms()
        sync.defer_all, sync.disabled = False, True
        none = mode_ms()
        sync.disabled = False
        total_comm, exposed = max(at_end - none, 0.0), max(overlapped - none, 0.0)
        ddp_info = {"n_ranks_seen": len({r[0] for r in ranks}), "devices": sorted({r[1] for r in ranks}), "backend": dist.get_backend(), "exchange_dtype": args.grad_exchange,
                    "exchange_algorithm": args.exchange, "collectives_per_step": n_coll,
                    # the RCCL knobs in force (passed through untouched: set them in the launching environment to A/B algorithms / protocols on a real node)
                    "rccl_env": {k: v for k, v in sorted(os.environ.items()) if k.startswith(("NCCL_", "RCCL_", "HSA_ENABLE_IPC", "HSA_FORCE_FINE_GRAIN"))},
                    "payload_bytes_per_step": payload_bytes, "early_collectives_per_step": n_early,
                    "graph": "identical to the N = 1 step: one grouped weight-gradient launch per block, the decoder's shared k|v GEMM with its parameters as a marked range of their own",
                    "ms_per_step_overlapped": round(overlapped, 3), "ms_per_step_exchange_after_backward": round(at_end, 3), "ms_per_step_no_exchange": round(none, 3),
                    "exposed_comm_ms": round(exposed, 3), "unoverlapped_comm_ms": round(total_comm, 3),
                    "hidden_fraction": (round(1.0 - exposed / total_comm, 3) if total_comm > 0 else None),
                    "how": "8 steps per mode after the timed region, max over ranks; per-collective kernel overlap: tools/rccl_overlap.py on a rocprofv3 kernel trace"}
    if world == 1 and args.force_sync and sync is not None:  # one-rank RCCL path check: what was issued in the last timed step
        ddp_info = {"n_ranks_seen": 1, "backend": dist.get_backend(), "exchange_dtype": args.grad_exchange, "exchange_algorithm": args.exchange,
                    "collectives_per_step": sync.n_collectives_last, "early_collectives_per_step": sync.n_early_last, "payload_bytes_per_step": sync.bytes_last,
                    "what": "--force-sync: a one-rank process group on RCCL; the overlapped schedule of the N > 1 step is issued, the mean is the identity"}
    # forward GFLOP of the reference graph x 3 (SURVEY appendix A probes): config 2 and config 5 shapes only
    ref_gflop = {("base", "192,192,16", "192,192"): STEP_GFLOP_PER_SAMPLE, ("large", "256,256,24", "256,256"): 3 * 1806.7}.get((args.size, args.sax, args.lax))
    step.replay = False  # the information-only runs below (dense stem, per-launch events) go through the module code

    # the same steps with the stem evaluated on every voxel like the reference (information only; single process)
    from cinema_amd import convvit
    dense_stem, dense_ms = convvit.DENSE_STEM, None
    if world == 1 and not dense_stem and args.profile_steps > 0:
        convvit.DENSE_STEM = True
        for i in range(2):
            step(batches[i % 2], 0.75)
        torch.cuda.synchronize()
        td = time.perf_counter()
        for i in range(args.steps):
            step(batches[i % 2], 0.75)
        torch.cuda.synchronize()
        dense_ms = round((time.perf_counter() - td) / args.steps * 1e3, 3)
        convvit.DENSE_STEM = False

    # ---- per-kernel roofline: time every GEMM launch with HIP events on the launch stream (extra steps, same workload)
    roofline = None
    if args.profile_steps > 0:  # EVERY rank steps (the steps contain the gradient collectives); only rank 0 records and reports
        from cinema_amd import tape as T_

        side, T_.SIDE_WGRAD = T_.SIDE_WGRAD, False  # one stream while timing single launches: a kernel sharing the chip with the
        step(batches[0], 0.75)                      # side-stream weight gradients would be charged for the overlap
        if rank == 0:
            K.GEMM_PROFILE = []
        for i in range(args.profile_steps):
            step(batches[i % 2], 0.75)
        barrier()
        prof, K.GEMM_PROFILE = K.GEMM_PROFILE, None
        T_.SIDE_WGRAD = side
    if rank == 0 and args.profile_steps > 0:
        agg: dict = {}
        for kind, flops, e0, e1, shape, *_ in prof:
            a = agg.setdefault(kind, [0.0, 0.0, 0, 0.0])
            a[0] += flops
            a[1] += e0.elapsed_time(e1) * 1e-3
            a[2] += 1
            a[3] += shape[-1]
        try:  # (information only: the headline line must not depend on it)
            blas = hipblaslt_reference(prof, args.profile_steps, K.GEMM_KERNEL_NAMES) if not args.no_blas_reference else {}
        except Exception:  # noqa: BLE001
            blas = {}
        kind = max(agg, key=lambda k: agg[k][1])
        flops, secs, n, alg_bytes = agg[kind]
        traffic = pmc_traffic(K.GEMM_KERNEL_NAMES[kind])
        achieved = flops / secs / 1e12
        dom = gemm_roof(flops, alg_bytes, secs)
        hbm_dom = dom["bound"] == "hbm"
        # the roof that bounds the dominant kernel follows from its algorithmic intensity (gemm_roof); `frac` is against that roof.  The AT-TRAFFIC intensity
        # (FLOP / PMC byte) says on which side of the ridge the kernel runs with the bytes it really moves
        roofline = {"bound": dom["bound"], "kernel": K.GEMM_KERNEL_NAMES[kind], "achieved": dom["alg_gb_s"] if hbm_dom else round(achieved, 1),
                    "peak": HBM_PEAK_GBS if hbm_dom else MFMA_BF16_PEAK_TFLOPS, "unit": "GB/s" if hbm_dom else "TFLOP/s", "frac": dom["frac"], "traffic": traffic,
                    "intensity_flop_per_byte": dom["intensity_flop_per_byte"], "ridge_flop_per_byte": round(RIDGE_FLOP_PER_BYTE, 1),
                    "intensity_at_measured_traffic": round(flops / n / traffic, 1) if traffic else None,
                    "algorithmic_bytes_per_launch": round(alg_bytes / n), "traffic_over_algorithmic": round(traffic / (alg_bytes / n), 2) if traffic else None,
                    "traffic_source": f"committed {PMC_TRAFFIC_FILE} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, tools/gpu_pmc_round.sh); not collected live",
                    "traffic_stale": pmc_binding(PMC_TRAFFIC_FILE)["stale"], "traffic_binding": pmc_binding(PMC_TRAFFIC_FILE),
                    "mfma_util": pmc_mfma_util(K.GEMM_KERNEL_NAMES[kind]),
                    "mfma_util_source": f"committed {PMC_MFMA_FILE} (SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE passes, tools/gpu_pmc_round.sh); not collected live",
                    "mfma_util_stale": pmc_binding(PMC_MFMA_FILE)["stale"],
                    "timing": "HIP events on the launch stream around every launch of this kernel, live in this process (a grouped persistent launch finishes its split reduction inside the kernel; for the 128x128 split-K kernel the events also cover the reduce launch behind it)",
                    "launches_per_step": n // args.profile_steps, "avg_launch_us": round(secs / n * 1e6, 2),
                    "gflop_per_launch": round(flops / n / 1e9, 3),
                    "all_gemm_kernels": {K.GEMM_KERNEL_NAMES[k]: {**gemm_roof(v[0], v[3], v[1]), "ms_per_step": round(v[1] / args.profile_steps * 1e3, 3),
                                                                  "launches_per_step": v[2] // args.profile_steps, **blas.get(K.GEMM_KERNEL_NAMES[k], {})} for k, v in agg.items()},
                    "vs_hipblaslt_note": "measurement only - the library never calls a BLAS: hipBLASLt (torch.mm) on the same problems (same m, n, k and operand layouts, bf16 result, NO "
                                         "epilogue, one call per problem back to back, idle chip) / this library's launch times inside the step (fused epilogues included); > 1 = faster than hipBLASLt",
                    "all_gemm_kernels_note": "bound / frac per instance from its algorithmic intensity (FLOP per algorithmic byte vs the 312.5 FLOP/B ridge of 2.5 PF / 8 TB/s): "
                                             "hbm-bound instances are priced against 8 TB/s, mfma-bound ones against 2.5 PF; frac_of_mfma_peak is kept for comparison with earlier rounds",
                    "hbm_kernels": hbm_kernel_rows(PMC_TRAFFIC_FILE)}

    if rank == 0:
        samples_per_s = world * args.batch * args.steps / dt
        out = {
            "metric": "MAE-pretrain samples/sec (4-view cine, 75% mask)", "value": round(samples_per_s, 2), "unit": "samples/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "untimed_steps": extra_untimed + args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": ("bf16" if args.dtype == "bf16" else "fp8 (OCP e4m3 forward, data-gradient and weight-gradient GEMMs of the transformer blocks: weights per tensor (current scaling), activations / gradients per tensor (delayed scaling))"), "data": "synthetic",
            "config": {"workload": f"CineMA ViT-{args.size.capitalize()} MAE, 4 views (SAX {args.sax.replace(',', 'x')} + LAX 2C/3C/4C {args.lax.replace(',', 'x')}), mask 0.75, "
                                   f"per-GPU batch {args.batch}, fwd+bwd+clip(5.0)+AdamW, random-init weights",
                       "global_batch": world * args.batch, "parallelism": f"dp{world}", "final_loss": round(final_loss, 5),
                       "stem": "dense (every voxel, as the reference)" if dense_stem else
                               "visible voxels only - exact: masked voxels never reach a kept token (DESIGN.md 3a); CINEMA_DENSE_STEM=1 runs every voxel",
                       "dense_stem_ms_per_step": dense_ms, "peak_mem_gib": peak_gib,
                       "host": ("module code issues every launch (--eager)" if args.eager else
                                f"forward+backward re-issued from a recorded list of {n_launches} entries (cinema_amd/replay.py: kernel launches, stream forks / joins, "
                                "lane-group markers - the entries of a lane group go out as ONE merged kernel per position); clip+AdamW eager"),
                       # kernels handed to the HIP runtime per timed step, counted by the library (cinema_kernel_launch_count): whole step incl. clip + AdamW
                       "kernel_launches_per_step": kernels_per_step,
                       # the REFERENCE's dense FLOP count per sample x samples/s: a reference-equivalent rate, not executed FLOPs
                       "reference_equiv_tflops_per_gpu": (None if ref_gflop is None else round(samples_per_s / world * ref_gflop / 1e3, 1))},
            "roofline": roofline,
        }
        if ddp_info is not None:
            out["ddp"] = ddp_info
        if world == 1 and args.cpu_budget > 0:
            out["cpu_baseline"], out["parity"] = cpu_baseline(kw, cpu_state, 2, args.cpu_budget, device)
        default_workload = (args.size, args.sax, args.lax, args.dtype, args.batch) == ("base", "192,192,16", "192,192", "bf16", 16)
        if world == 1 and default_workload and not args.no_secondary and not args.force_sync and args.profile_steps > 0:
            import gc

            del step, model, batches
            gc.collect()
            torch.cuda.empty_cache()
            try:
                out["secondary"] = secondary_configs(device, with_parity=args.cpu_budget > 0)
            except Exception as e:  # noqa: BLE001  (the headline line must not depend on the information-only runs)
                out["secondary"] = {"error": f"{type(e).__name__}: {e}"}
            b64 = out["secondary"].get("config2_global_batch_64") if isinstance(out["secondary"], dict) else None
            if b64 is not None:
                # batch-independent part of the step: the marginal cost per sample from the two batch sizes of this run, (ms64 - ms16) / 48, extrapolated to batch 0
                per_sample = (b64["ms_per_step"] - out["ms_per_step"]) / 48.0
                out["config"]["fixed_ms_per_step"] = round(out["ms_per_step"] - 16.0 * per_sample, 3)
                out["config"]["marginal_ms_per_sample"] = round(per_sample, 4)
        emit(out, args.details)
    if world > 1 or args.force_sync:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

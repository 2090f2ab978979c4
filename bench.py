#!/usr/bin/env python
"""bench.py -- attack iterations/sec of the MI355X hot path, with roofline and CPU-baseline legs.

Contract (driver):  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  A plain run sets up, warms up, times the K steps and prints the one JSON line (headline value, ms_per_step, the device span of
  kernel A's forward launches inside the timed region); every other leg described below -- the event-timed kernel figures, the
  BERT-base and read-ceiling probes, live PMC, restarts32, the selection collectives, parity and both baselines -- runs only with
  --full (their fields are null otherwise).  --dump-outputs DIR writes what the timed path computed in its last step (see
  dump_outputs) before any of those legs touches the trial state; such a run uses deterministic convolution solvers chosen without
  timing throughout (see main), so two runs with the same arguments write the same files.
  N > 1: the driver launches it through torch.distributed.run (one rank per GPU); a bare `python bench.py --gpus N` re-launches
  itself the same way.  With fewer GPUs than ranks (a 1-GPU box) the ranks share devices and agree over gloo -- a functional
  check only, flagged "oversubscribed": true.

  * workload = BASELINE.json configs[1]: ResNet-18 (1000 classes, random init), ImageNet-shaped 1x3x224x224 candidate,
    attack=invertinggradients (cosine-similarity gradient matching + TV 0.2, hard-sign Adam lr 0.1, box projection,
    step-lr schedule of the full 24 000-iteration run).  Synthetic data, inputs resident in HBM before timing starts.
  * a "step" = one attack iteration (`optimizer.step(closure)` of optimization_based_attack.py:110-121): victim
    forward + backward + double backward on PyTorch-ROCm, kernels A/B/C of libbreach_hip.so for everything else.
  * N GPUs = N independent restarts (trials), one per rank (weak scaling); value = N*K / max-over-ranks wall time.
    After the timed region the ranks agree on the best trial with ONE all-reduce(MIN) + one broadcast (RCCL).
  * roofline: the fused gradient-matching reduction (kernel A forward, gm_fwd_kernel): algorithmic bytes 2*N*4 per launch
    over the average launch duration measured with HIP events (hipExtLaunchKernelGGL start/stop = the dispatch's own
    timestamps) on the launch stream; `stage_*` adds the one-workgroup finalize launch; `timed_region_span_*` is the device
    wall-clock span of the forward launches inside the timed graph-replay region.
    `roofline.hbm_resident`: the same kernels timed in the same run on a synthetic list of BERT-base's 201 gradient tensors
    (86.07 M elements, 688.6 MB per forward launch -- 2.7x the 256 MiB Infinity Cache, so this is an HBM figure, which the
    ResNet-18 list's is not).
    `roofline.traffic`: HBM bytes per launch from rocprofv3 PMC passes (FETCH_SIZE x 2 + WRITE_SIZE, separate passes) collected IN THIS
    RUN, after the timed region, over scripts/pmc_target.py (N = 1; the committed passes are the fall-back, `traffic_source` says which).
    `roofline.ceiling`: what a launch shaped like kernel A's forward (same persistent grid, same eight staged 16-byte loads
    per lane, two multiply-adds per element instead of the objective; scripts/diag/read_ceiling.hip, NOT part of the library)
    reaches on buffers of the same size in this run, right behind a writer -- for a list that streams from the 256 MiB
    Infinity Cache (ResNet-18's does) the 8 TB/s HBM peak is the wrong denominator, this is the measured one.
  * parity: teacher-forced evaluations of the timed configuration at the reference's own late iterate (k = 23 991 of the
    24 000-iteration CPU run of the unmodified reference, tests/golden/attack_resnet18_24k.npz) -- loss and step direction of the timed
    path, of a PyTorch-ROCm-only control on the same GPU, and kernels A / C against torch ops on the SAME inputs (`parity_leg`).
  * restarts32: BASELINE configs[3] through the product entry -- `attacker.reconstruct` with restarts.num_trials = 32 on the headline
    workload, wall time incl. rescoring and selection: at N = 1 in this process (8 groups of 4 trials in flight), at N > 1 through the
    product's TrialWorkerPool from rank 0 in a bounded process of its own after the ranks have left (`restarts32_leg`).
  * gpu_torch_baseline: the same attack with PyTorch-ROCm ops for the attack-side arithmetic (oracle/restate.py on the GPU, no
    kernel of libbreach_hip.so), a bounded number of iterations: what the HIP path buys ON THIS CHIP.  A reported baseline.
  * cpu_baseline: the UNMODIFIED reference through oracle/ref_shim.py when a reference checkout is importable
    (`kind: "reference"`; /root/reference in the build container, BREACHING_REFERENCE elsewhere), else oracle/restate.py (CPU
    restatement pinned to the reference by tests/test_oracle_pinning.py; `kind: "port"`, with the committed port / reference
    anchor ratio next to it) -- on the host cores, same workload, a bounded number of iterations, rank 0 at N=1 only.
"""

import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # one hardware queue per trial in flight (see breaching_amd/__init__.py)

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def pmc_traffic_bytes(kernel, sources=None):
    """HBM bytes per launch from the committed PMC passes (profiles/r*_pmc_{fetch,write}_pmc_summary.csv, the newest of
    each): FETCH_SIZE (KB) x 2 -- the gfx950 half-count of wide coalesced reads, MI355X_MICROARCH.md section HBM -- plus
    WRITE_SIZE (KB).  bench.py cannot collect counters itself: separate `rocprofv3 --pmc` passes do, one counter per pass,
    over scripts/pmc_target.py at this workload's list size (scripts/gpu_call.sh pmc_resnet18; under the full attack loop
    rocprofv3's counter collection segfaults inside torch's convolution on this image).  None when the profiles are absent.
    `sources` (a list) receives the file names used."""
    import csv
    import glob

    total = 0.0
    found = 0
    for counter, factor in (("fetch", 2.0), ("write", 1.0)):
        paths = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_{counter}_pmc_summary.csv")))
        if not paths:
            return None
        with open(paths[-1]) as f:
            for row in csv.DictReader(f):
                if row["kernel"].startswith(kernel):
                    total += float(row["avg_value"]) * 1024.0 * factor
                    found += 1
                    if sources is not None:
                        sources.append(os.path.basename(paths[-1]))
                    break
    return int(total) if found == 2 else None


def pmc_traffic_live(size="resnet18", timeout=90):
    """HBM bytes per launch of kernel A, collected NOW: two bounded subprocesses, `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE`
    (separate passes, counters only -- no tracing in the same run, as MI355X_MICROARCH.md's HBM section prescribes), over
    scripts/pmc_target.py: kernel A forward / finalize / backward alone on a synthetic list of this workload's size (under the full
    attack loop rocprofv3's counter collection segfaults inside torch's convolution on this image).  Returns
    {"gm_fwd_kernel": bytes, "gm_bwd_kernel": bytes} (FETCH_SIZE x 2 -- the gfx950 half-count of wide coalesced reads -- plus
    WRITE_SIZE, values in KiB) or None when rocprofv3 is absent or a pass fails; the caller then falls back to the committed passes."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    per = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
        try:
            cmd = [rocprof, "--pmc", counter, "--output-format", "csv", "-d", tmp, "--", sys.executable,
                   os.path.join(ROOT, "scripts", "pmc_target.py"), "--size", size, "--reps", "4"]
            proc = subprocess.run(cmd, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"}, capture_output=True, text=True, timeout=timeout)
            files = glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True)
            if proc.returncode != 0 or not files:
                return None
            sums = {}
            with open(files[0]) as f:
                for row in csv.DictReader(f):
                    if row.get("Counter_Name") != counter:
                        continue
                    for key in ("gm_fwd_kernel", "gm_bwd_kernel"):
                        if key in row["Kernel_Name"]:
                            sums.setdefault(key, []).append(float(row["Counter_Value"]))
            for key, values in sums.items():
                per.setdefault(key, {})[counter] = sum(values) / len(values)
        except Exception:
            return None
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for key, c in per.items():
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            out[key] = int((2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0)
    return out or None


def committed_replay_duration(kernel_prefix):
    """Average dispatch duration (us) of a kernel INSIDE the replayed hipGraph, from the newest committed rocprofv3 kernel trace of this
    bench command (profiles/r*_bench_kernel_summary.txt).  bench.py's own event pairs ride on eager launches -- a replayed graph cannot
    carry them -- and the same kernels run ~7 % faster inside the replay (no idle gaps between dispatches); rocprofv3 of the eager
    bench agrees with the events within 1 % (profiles/r5_bench_eager_kernel_summary.txt).  None when no trace is committed."""
    import glob
    import re

    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_kernel_summary.txt")))
    if not paths:
        return None, None
    with open(paths[-1]) as f:
        for line in f:
            if line.startswith(kernel_prefix):
                m = re.search(r"avg=\s*([0-9.]+)us", line)
                if m:
                    return float(m.group(1)), os.path.basename(paths[-1])
    return None, None


def device_record(device, clocks=True):
    """Which GPU and software produced the line (box-to-box differences of a few per cent come with MIOpen's timing-based solver
    choice on a fresh box and with the board; this is what a reader needs to tell two lines apart).  `clocks`: also query the
    current clock levels (a rocm-smi subprocess; --full runs only)."""
    import torch

    try:
        props = torch.cuda.get_device_properties(device)
        record = dict(name=props.name, arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count,
                      memory_GB=round(props.total_memory / 1e9, 1), torch=torch.__version__, hip=getattr(torch.version, "hip", None))
        try:  # current clock levels, when rocm-smi is there: the first thing to look at when two boxes differ by a few per cent
            if not clocks:
                return record
            import shutil
            import subprocess

            smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
            out = subprocess.run([smi, "--showclocks", "--json"], capture_output=True, text=True, timeout=20)
            if out.returncode == 0 and out.stdout.strip().startswith("{"):
                cards = json.loads(out.stdout)
                card = cards.get(f"card{device.index or 0}") or next(iter(cards.values()))
                record["clocks"] = {k: v for k, v in card.items() if "clock" in k.lower()}
        except Exception:
            pass
        return record
    except Exception as exc:  # provenance only: never fatal
        return dict(error=repr(exc)[:200])


def bert_base_gradient_shapes():
    """The 201 gradient tensors a TAG attack on BERT-base (MLM head, vocabulary 30 522) matches: every parameter but the
    word-embedding matrix (base_attack.py:94 pops it).  86 073 402 elements (SURVEY.md section 8 size table)."""
    H, I, V = 768, 3072, 30522
    shapes = [(512, H), (2, H), (H,), (H,)]  # position / token-type embeddings, embedding LayerNorm
    for _ in range(12):
        shapes += [(H, H), (H,)] * 4 + [(H,), (H,)] + [(I, H), (I,), (H, I), (H,)] + [(H,), (H,)]
    shapes += [(H, H), (H,), (H,), (H,), (V,)]  # MLM transform, its LayerNorm, decoder bias (decoder weight is tied)
    return shapes


def hbm_resident_leg(device, reps=30):
    """Kernel A forward / finalize / backward with hipExtLaunchKernelGGL events on a list that cannot sit in the Infinity Cache."""
    import torch

    from breaching_amd import _lib
    from breaching_amd.gm import GradientMatchPlan

    shapes = bert_base_gradient_shapes()
    gen = torch.Generator(device="cpu").manual_seed(0)
    data = [torch.randn(s, generator=gen).to(device) for s in shapes]
    rec = [torch.randn(s, generator=gen).to(device) for s in shapes]
    plan = GradientMatchPlan(data)
    n = plan.total_elements
    out = dict(list=f"BERT-base gradient list without the word embedding: {len(shapes)} tensors, {n} elements "
                    f"({2 * n * 4 / 1e6:.1f} MB per forward launch)", elements=n, measured="hipExtLaunchKernelGGL start/stop events, "
               f"{reps} back-to-back forward + finalize + backward triples on the current stream, the 5 slowest dropped")
    for kind_name in ("cosine-similarity", "tag-euclidean"):
        kind = _lib.GM_KINDS[kind_name]
        weights = torch.linspace(1, 0.1, len(shapes), device=device) if kind_name == "tag-euclidean" else None
        for _ in range(3):
            plan.backward(kind, rec, plan.forward(kind, rec, 1.0, 0.1, 1e-7, weights), None, weights)
        plan.enable_timing()
        for _ in range(reps):
            plan.backward(kind, rec, plan.forward(kind, rec, 1.0, 0.1, 1e-7, weights), None, weights)
        torch.cuda.synchronize(device)
        t = plan.drain_timers()
        f, e, b = (sum(sorted(t[k])[:-5]) / (len(t[k]) - 5) for k in ("fwd", "fin", "bwd"))
        spread = {k: dict(min=round(min(t[k]), 2), median=round(sorted(t[k])[len(t[k]) // 2], 2), max=round(max(t[k]), 2)) for k in ("fwd", "bwd")}
        # the same forward launch with nothing but its own finalize between repetitions: in the triple above every forward
        # follows a backward that has just written 344 MB, whose write-back competes with the forward's reads (the in-loop
        # condition: there autograd has just written the reconstructed list)
        plan.enable_timing()
        for _ in range(reps):
            plan.forward(kind, rec, 1.0, 0.1, 1e-7, weights)
        torch.cuda.synchronize(device)
        alone = plan.drain_timers()["fwd"]
        fa = sum(sorted(alone)[:-5]) / (len(alone) - 5)
        out[kind_name] = dict(fwd_us=round(f, 2), finalize_us=round(e, 2), bwd_us=round(b, 2),
                              fwd_GBs=round(2 * n * 4 / f / 1e3, 1), frac=round(2 * n * 4 / f / 1e3 / HBM_PEAK_GBS, 4),
                              stage_frac=round(2 * n * 4 / (f + e) / 1e3 / HBM_PEAK_GBS, 4),
                              bwd_GBs=round(3 * n * 4 / b / 1e3, 1), bwd_frac=round(3 * n * 4 / b / 1e3 / HBM_PEAK_GBS, 4),
                              fwd_not_behind_a_writer_us=round(fa, 2), frac_not_behind_a_writer=round(2 * n * 4 / fa / 1e3 / HBM_PEAK_GBS, 4),
                              fwd_us_min_median_max=spread["fwd"], bwd_us_min_median_max=spread["bwd"],
                              frac_at_min_us=round(2 * n * 4 / spread["fwd"]["min"] / 1e3 / HBM_PEAK_GBS, 4),
                              frac_at_median_us=round(2 * n * 4 / spread["fwd"]["median"] / 1e3 / HBM_PEAK_GBS, 4))
    plan.timers = None
    return out


def read_ceiling_leg(device, n_elements, kernel_us, reps=30):
    """The measured ceiling of a launch shaped like kernel A's forward at this list size: scripts/diag/read_ceiling.hip (a
    diagnostic kernel OUTSIDE libbreach_hip.so: kernel A's persistent grid of 512 workgroups and eight staged 16-byte loads per
    lane over two buffers, two multiply-adds per element), each launch right behind a kernel that has just rewritten the first
    buffer (what autograd does to the reconstructed gradient list), timed with the dispatch's own start / stop events."""
    import ctypes
    import subprocess

    import torch

    from breaching_amd import _lib

    src = os.path.join(ROOT, "scripts", "diag", "read_ceiling.hip")
    lib_path = os.path.join(ROOT, "scripts", "diag", "libread_ceiling.so")
    if not os.path.exists(lib_path) and os.path.exists(src):  # built in-tree by __graft_entry__.build(); last resort here
        subprocess.run([os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                        src, "-o", lib_path], check=True, capture_output=True)
    diag = ctypes.CDLL(lib_path)
    diag.diag_read_timed.restype = ctypes.c_int
    diag.diag_read_timed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]
    n_chunks = n_elements // 4096
    a, b = torch.randn(n_chunks * 4096, device=device), torch.randn(n_chunks * 4096, device=device)
    sink = torch.zeros(4096, device=device)
    nbytes = 2 * n_chunks * 4096 * 4
    stream = _lib.current_stream_handle(device)
    out = dict(kind="read probe with kernel A's grid and loads (scripts/diag/read_ceiling.hip, outside the library), each launch behind a "
                    "writer of the first buffer; dispatch start/stop events", bytes=nbytes)
    for tag, fill in (("behind_writer", 1), ("warm", 0)):
        us = (ctypes.c_float * (reps + 5))()
        rc = diag.diag_read_timed(a.data_ptr(), b.data_ptr(), n_chunks, 512, 0, sink.data_ptr(), stream, fill, reps + 5, us)
        if rc != 0:
            return dict(error=f"diag_read_timed returned {rc}")
        t = sorted(us[5:])
        out[tag] = dict(min_us=round(t[0], 2), median_us=round(t[len(t) // 2], 2), max_us=round(t[-1], 2),
                        GBs=round(nbytes / t[len(t) // 2] / 1e3, 1), frac_of_hbm_peak=round(nbytes / t[len(t) // 2] / 1e3 / HBM_PEAK_GBS, 4))
    out["us"], out["GBs"] = out["behind_writer"]["median_us"], out["behind_writer"]["GBs"]
    out["kernel_A_forward_over_ceiling"] = round(out["us"] / kernel_us, 4)  # 1.0 = kernel A's forward takes what the bare read takes
    return out


def parity_leg(device, model_name):
    """The timed configuration against the unmodified reference, in one evaluation: at the reference's own iterate x_k of its
    24 000-iteration CPU run (the latest stored one, k = 23 991; tests/golden/attack_resnet18_24k.npz, written by
    oracle/make_golden.py golden_resnet18_24k) the objective and sign(d total / dx) -- what hard-sign Adam consumes -- against the
    reference's history[k] and sign map, next to the reference's OWN agreement with itself when x_k moves by <= 16 ulp.

    So that a deviation from the CPU reference has an owner, on this GPU in this run:
      * `control`      the evaluation with PyTorch-ROCm ops only -- oracle/restate.py's statements (the checker, pinned to the reference
                       by tests/test_oracle_pinning.py), torch's own BatchNorm; no kernel of libbreach_hip.so.  Its deviation from the CPU
                       reference is the victim's convolutions on MIOpen instead of oneDNN at a kink-dense late iterate.
      * `kernels_A_C`  kernel A behind the double backward + kernel C on the STOCK BatchNorm modules (a victim pass of its own);
        the timed path the same with kernel E (eval BatchNorm as y = x * s_c + t_c).
      * `kernels_on_the_same_inputs`  kernel A (value and backward) and kernel C against the restatement's torch ops on the SAME
                       reconstructed gradient list and the same x_k: the comparison no vendor-library choice can enter.  Held to
                       north_star's 1e-4 outright (measured: 1e-7).
    The full evaluations are each held to max(1e-4, 3 x the fixture's 16-ulp sensitivity): round 6 found that two victim passes of the
    same expression in one process agree to 2e-7 or differ by 3-7e-4 depending on what ran before (MIOpen) -- control and HIP path alike."""
    import copy

    import numpy as np
    import torch

    import breaching_amd
    from breaching_amd.cases import build_case, parameter_checksum
    from oracle import restate

    path = os.path.join(ROOT, "tests", "golden", "attack_resnet18_24k.npz")
    if model_name != "resnet18" or not os.path.exists(path):
        return None
    gold = np.load(path)
    case = build_case("resnet18", "ImageNet", 1, device=device)  # observed gradient computed on the CPU: the target the reference attacked
    if abs(parameter_checksum(case.model) / float(gold["model_checksum"]) - 1) > 1e-10:
        return dict(error="model of this run differs from the fixture's")
    i = int(np.argmax(gold["forced_k"]))
    k = int(gold["forced_k"][i])
    sign_ref = torch.as_tensor(gold["forced_sign"][i].astype(np.float32))
    weight = torch.as_tensor((gold["forced_grad_bf16"][i].astype(np.uint32) << 16).view(np.float32)).abs().double()
    want = float(gold["history"][k])

    def against_reference(total, grad):
        same = (torch.sign(grad.detach().cpu()) == sign_ref).double()
        return dict(loss=float(total.detach()), loss_rel_err=abs(float(total.detach()) - want) / want, sign_agreement=float(same.mean()),
                    weighted_sign_agreement=float((same * weight).sum() / weight.sum()))

    def hip_evaluation(extra):
        cfg = breaching_amd.get_attack_config("invertinggradients", [f"optim.max_iterations={int(gold['iterations'])}"] + extra)
        attacker = breaching_amd.prepare_attack(case.model, case.loss_fn, cfg, dict(device=device, dtype=torch.float))
        shared = [dict(gradients=list(d["gradients"]), buffers=d["buffers"], metadata=dict(d["metadata"])) for d in case.shared_data]
        rec_models, labels, _ = attacker.prepare_attack(case.server_payload, shared)
        for reg in attacker.regularizers:
            reg.initialize(rec_models, shared, labels)
        attacker.objective.initialize(attacker.loss_fn, cfg.impl, None)
        attacker.objective.prepare(rec_models, shared)
        xk = torch.as_tensor(gold["forced_x"][i]).to(device).clone().requires_grad_(True)
        total, _ = attacker._autograd_objective([xk], labels, rec_models, shared, attacker.regularizers)
        (g,) = torch.autograd.grad(total, [xk])
        return cfg, labels, total.detach(), g.detach()

    cfg, labels, total, g = hip_evaluation([])                                   # the timed path
    _, _, total_ac, g_ac = hip_evaluation(["impl.fast_eval_bn=False"])           # kernels A and C on the stock BatchNorm modules
    control_model = copy.deepcopy(case.model).to(device).eval()
    data = [t.to(device) for t in case.shared_data[0]["gradients"]]
    xc = torch.as_tensor(gold["forced_x"][i]).to(device).clone().requires_grad_(True)
    task = case.loss_fn(control_model(xc), labels)
    rec_grads = torch.autograd.grad(task, tuple(control_model.parameters()), create_graph=True)
    control_total = restate.gradient_objective("cosine-similarity", rec_grads, data, cfg.objective)
    control_total = control_total + restate.total_variation(xc, **cfg.regularization["total_variation"])
    (gc,) = torch.autograd.grad(control_total, [xc])
    control = against_reference(control_total, gc)
    control["what"] = ("the same evaluation on this GPU with PyTorch-ROCm ops only (oracle/restate.py statements, torch BatchNorm): the "
                       "victim's convolutions as in the HIP path, no kernel of libbreach_hip.so")
    kernels_ac = against_reference(total_ac, g_ac)
    kernels_ac.update(what="kernel A (behind the double backward) + kernel C on the stock BatchNorm modules (impl.fast_eval_bn=False), a victim pass "
                           "of its own", loss_vs_control_rel=abs(float(total_ac) - float(control_total.detach())) / abs(float(control_total.detach())),
                      sign_agreement_vs_control=float((torch.sign(g_ac.cpu()) == torch.sign(gc.detach().cpu())).double().mean()))
    # Kernels A and C against torch ops ON THE SAME INPUTS -- the control's own reconstructed gradient list (one victim pass, shared) and
    # x_k: the one comparison on this GPU that vendor-library algorithm choices cannot enter.  Value, and the gradient kernel A's
    # backward hands to the double backward (max deviation over all 11.7 M elements, relative to the largest element).
    from breaching_amd.gm import objective_lookup as hip_objectives
    from breaching_amd.priors import HipTotalVariation

    def value_and_gradients(objective_fn, inputs):
        leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
        value = objective_fn(leaves)
        return value.detach().reshape(-1)[0], [t.detach() for t in torch.autograd.grad(value.sum(), leaves)]

    hip_objective = hip_objectives[cfg.objective.type](**cfg.objective)
    hip_objective.initialize(case.loss_fn, cfg.impl, None)
    v_t, g_t = value_and_gradients(lambda rec: restate.gradient_objective("cosine-similarity", rec, data, cfg.objective), rec_grads)
    v_h, g_h = value_and_gradients(lambda rec: hip_objective.gradient_based_loss(rec, data), rec_grads)
    peak = max(float(t.abs().max()) for t in g_t)
    tv_t, tvg_t = value_and_gradients(lambda xs: restate.total_variation(xs[0], **cfg.regularization["total_variation"]), [xc])
    tv_h, tvg_h = value_and_gradients(lambda xs: HipTotalVariation(dict(device=device, dtype=torch.float), **cfg.regularization["total_variation"])(xs[0]), [xc])
    same_inputs = dict(
        what="kernel A (value + backward) and kernel C (value + gradient) against oracle/restate.py's torch statements on the SAME inputs: the "
             "control's reconstructed gradient list (62 tensors, 11.7 M elements) and x_k -- no victim pass in between, nothing vendor-chosen",
        gm_value_rel=abs(float(v_h) - float(v_t)) / abs(float(v_t)),
        gm_gradient_max_dev_over_peak=max(float((a - b).abs().max()) for a, b in zip(g_h, g_t)) / peak,
        tv_value_rel=abs(float(tv_h) - float(tv_t)) / abs(float(tv_t)),
        tv_gradient_max_dev_over_peak=float((tvg_h[0] - tvg_t[0]).abs().max()) / float(tvg_t[0].abs().max()), tolerance=1e-4)
    same_inputs["ok"] = bool(max(same_inputs["gm_value_rel"], same_inputs["gm_gradient_max_dev_over_peak"], same_inputs["tv_value_rel"],
                                 same_inputs["tv_gradient_max_dev_over_peak"]) <= same_inputs["tolerance"])
    sensitivity = float(gold["forced_sensitivity"][i])
    ref_psnr = np.concatenate([[gold["psnr"]], gold["twin_psnr"]])
    timed = against_reference(total, g)
    tolerance = max(1e-4, 3.0 * sensitivity)
    out = dict(fixture="tests/golden/attack_resnet18_24k.npz (unmodified reference on CPU, 24 000 iterations)", iterate=k,
               loss_reference=want, loss_hip=timed["loss"], loss_rel_err=timed["loss_rel_err"], loss_tolerance=tolerance,
               loss_tolerance_is="max(1e-4, 3 x kink_sensitivity_recorded) for EVERY full evaluation on this GPU, the control included: a victim pass "
                                 "goes through MIOpen, whose algorithm choice is not a function of the problem alone -- two evaluations of the same "
                                 "expression in one process agree to 2e-7 or differ by 3-7e-4 here depending on what ran before (round 6: seen on the "
                                 "control and on the HIP path alike) -- and the fixture's sensitivity is what an ulp-level perturbation does to the "
                                 "reference itself at this iterate.  What the attack-side kernels add is `kernels_on_the_same_inputs`, held to 1e-4 outright",
               control=control, kernels_A_C=kernels_ac, kernels_on_the_same_inputs=same_inputs,
               loss_hip_vs_control_rel=abs(timed["loss"] - float(control_total.detach())) / abs(float(control_total.detach())),
               kink_sensitivity_recorded=sensitivity,
               sign_agreement=timed["sign_agreement"], reference_twin_agreement=float(gold["forced_twin_sign_agreement"][i]),
               weighted_sign_agreement=timed["weighted_sign_agreement"],
               reference_twin_weighted_agreement=float(gold["forced_twin_weighted_sign_agreement"][i]),
               psnr_db_reference_runs=dict(mean=round(float(ref_psnr.mean()), 4), n=int(len(ref_psnr))))
    out["ok"] = bool(same_inputs["ok"] and max(out["loss_rel_err"], control["loss_rel_err"], kernels_ac["loss_rel_err"]) <= tolerance
                     and 1 - out["sign_agreement"] <= 3 * (1 - out["reference_twin_agreement"]) + 1e-3)
    hip_runs = os.path.join(ROOT, "profiles", "r5_config1_24k_8starts.json")  # free-running HIP runs of the full horizon (committed)
    if os.path.exists(hip_runs):
        try:
            with open(hip_runs) as f:
                rec = json.load(f)
            out["from_committed_profiles"] = dict(psnr_db_hip_runs=dict(mean=round(float(np.mean(rec["hip"]["psnr_db"])), 4), n=len(rec["hip"]["psnr_db"]),
                                                                         file="profiles/r5_config1_24k_8starts.json", note="not measured in this run"))
        except Exception:
            pass
    return out


def gpu_torch_baseline_leg(device, model_name, iters):
    """The same attack on the same GPU with PyTorch-ROCm ops for everything: oracle/restate.py (the statement-by-statement
    restatement of the reference loop) with device = cuda.  Same victim model arithmetic as the HIP path; about 1.5 k ATen launches
    per iteration for the attack-side arithmetic instead of kernels A / B / C.  Eager, one process, `iters` iterations after 3."""
    import torch

    import breaching_amd
    from breaching_amd.cases import build_case, initial_candidate
    from oracle import restate

    case = build_case(model_name, "ImageNet", 1, device=device, gradient_device=device)
    cfg = breaching_amd.get_attack_config("invertinggradients")
    x0 = initial_candidate(case.data_cfg, 1)
    restate.run_attack(case.model, case.loss_fn, cfg, case.server_payload, case.shared_data, initial_data=x0, max_iterations=3, device=device)
    torch.cuda.synchronize(device)
    timing = []
    _, stats = restate.run_attack(case.model, case.loss_fn, cfg, case.server_payload, case.shared_data, initial_data=x0, max_iterations=iters,
                                  device=device, timing=timing)
    return dict(value=round(iters / timing[0], 3), unit="attack iterations/s", kind="port on the GPU (oracle/restate.py, PyTorch-ROCm ops, eager)",
                sample=f"{iters} iterations of the same {model_name}/224 invertinggradients workload after 3 warm-up iterations; the loop "
                       "synchronises once per iteration (`.item()` of the loss), as the reference's does",
                final_objective=stats["Trial_0_Val"][-1])


def cpu_anchor_ratio():
    """port / reference iterations-per-second ratio from the committed anchor measurements (scripts/cpu_baseline_anchor.py:
    the unmodified reference and oracle/restate.py timed on the same threads in the build container), newest file."""
    import glob

    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_cpu_baseline_anchor.json")))
    if not paths:
        return None
    try:
        with open(paths[-1]) as f:
            rec = json.load(f)
        return dict(port_over_reference=rec.get("port_over_reference"), file=os.path.basename(paths[-1]), threads=rec.get("threads"))
    except Exception:
        return None


def cpu_baseline_leg(model_name, iters, cpu_threads=0):
    """The reference's CPU path on this box's host cores, same workload, `iters` loop iterations.  kind "reference": the
    UNMODIFIED reference through oracle/ref_shim.py when a checkout is importable (a (2 + iters)-iteration reconstruct() minus a
    2-iteration one isolates the loop from the model rebuild and the final rescoring, as scripts/cpu_baseline_anchor.py does);
    kind "port": oracle/restate.py, with the committed port / reference anchor ratio next to it.  Needs no GPU."""
    import torch

    import breaching_amd
    from breaching_amd.cases import build_case, initial_candidate

    host_cores = os.cpu_count() or 1
    # torch's CPU convolutions at B = 1 peak at 16 threads on the 256-logical-core host of the GPU box and LOSE beyond it
    # (profiles/r4_cpu_thread_sweep.json: 8 / 16 / 32 / 64 / 128 threads = 15.7 / 18.3 / 8.3 / 3.3 / 0.9 it/s): the baseline is
    # timed at its best thread count, not at os.cpu_count(); --cpu-threads overrides
    threads = cpu_threads if cpu_threads > 0 else min(host_cores, 16)
    torch.set_num_threads(threads)
    cpu_case = build_case(model_name, "ImageNet", 1, device="cpu")
    x0_cpu = initial_candidate(cpu_case.data_cfg, 1)
    reference_root = os.environ.get("BREACHING_REFERENCE", "/root/reference")
    kind, seconds, note = "port", None, None
    if os.path.isdir(os.path.join(reference_root, "breaching")):
        try:  # the unmodified reference, exactly as oracle/make_golden.py runs it
            from oracle.make_golden import _cfg as reference_cfg
            from oracle.make_golden import _run_reference_attack

            def timed_reference(its):
                tc = time.perf_counter()
                _run_reference_attack(reference_cfg("invertinggradients", [f"optim.max_iterations={its}", "optim.callback=100000"]), cpu_case, x0_cpu)
                return time.perf_counter() - tc

            timed_reference(2)  # warm-up: allocator, oneDNN primitives, TorchScript
            short = timed_reference(2)
            seconds, kind = timed_reference(2 + iters) - short, "reference"
            note = (f"{iters} loop iterations of the same {model_name}/224 invertinggradients workload through the UNMODIFIED reference "
                    f"({reference_root} via oracle/ref_shim.py; torch {torch.__version__} CPU): a (2 + {iters})-iteration reconstruct() minus "
                    "a 2-iteration one, after a warm-up call")
        except Exception as exc:
            note = f"reference checkout found but not runnable ({exc!r}); "
    if seconds is None:
        from oracle import restate

        cpu_cfg = breaching_amd.get_attack_config("invertinggradients")
        restate.run_attack(cpu_case.model, cpu_case.loss_fn, cpu_cfg, cpu_case.server_payload, cpu_case.shared_data,
                           initial_data=x0_cpu, max_iterations=2)  # warm-up (allocator, oneDNN primitives)
        timing = []
        restate.run_attack(cpu_case.model, cpu_case.loss_fn, cpu_cfg, cpu_case.server_payload, cpu_case.shared_data,
                           initial_data=x0_cpu, max_iterations=iters, timing=timing)
        seconds = timing[0]
        note = (note or "") + (f"{iters} iterations of the same {model_name}/224 invertinggradients workload through oracle/restate.py (torch "
                               f"{torch.__version__} CPU; no reference checkout on this box), after 2 warm-up iterations")
    out = dict(value=round(iters / seconds, 3), unit="attack iterations/s", cores=threads, host_cpu_count=host_cores, kind=kind, sample=note)
    if kind == "port":
        out["anchor"] = cpu_anchor_ratio()  # how the port relates to the unmodified reference on equal threads
    return out


def restarts32_leg(device, model_name, iters, num_trials=32, pool_world=0, committed_one_gpu=True):
    """BASELINE configs[3] through the PRODUCT entry: `attacker.reconstruct(server_payload, shared_data)` with restarts.num_trials
    = 32 on the headline workload -- the loop being sharded is optimization_based_attack.py:70-78, scoring :191-204, selection
    :206-218 -- wall seconds of the whole call incl. rescoring every trial and the selection.  Horizon shortened to `iters`
    iterations per trial (the step-lr milestones scale with it; stated in the record).  Two shapes, one function:
      * `pool_world` <= 1: one process, one GPU: 32 / 4 = 8 groups of four trials in flight (the one-GPU denominator of the 6x claim);
      * `pool_world` > 1: the single-process entry on a node -- this process is rank 0 and starts a `TrialWorkerPool` of pool_world - 1
        worker processes ("nccl" = RCCL over xGMI when every rank has its own GPU, gloo when ranks share one: `oversubscribed`),
        ships the inputs by broadcast, runs its own share four in flight, waits, selects with one all-reduce(MIN) + one broadcast:
        what `simulate_breach.py` gets on an 8-GPU node without changing a line.  Needs a process without a process group.
    A `dryrun=True` call (one iteration per trial) comes first in both shapes: pool start, MIOpen solver look-ups and the stream
    calibration stay out of the timed call and are reported beside it."""
    import torch

    import breaching_amd
    from breaching_amd.cases import build_case, psnr

    overrides = [f"restarts.num_trials={num_trials}", f"optim.max_iterations={iters}",
                 "impl.hip_graph=" + ("required" if pool_world <= 1 else "auto")]
    oversubscribed = False
    if pool_world > 1:
        have = torch.cuda.device_count()
        oversubscribed = have < pool_world
        own = device.index or 0
        devices = [own] + ([i for i in range(have) if i != own][: pool_world - 1] if not oversubscribed else [own] * (pool_world - 1))
        overrides += [f"impl.trial_devices={devices}", "impl.trial_pool=required"]
    else:
        devices = [device.index or 0]  # this process's own GPU only: no pool
        overrides += [f"impl.trial_devices={devices}"]
    os.environ["BREACH_HIP_TRIAL_DEVICES"] = ",".join(str(d) for d in devices)  # the environment outranks the config: say it there too
    cfg = breaching_amd.get_attack_config("invertinggradients", overrides)
    case = build_case(model_name, "ImageNet", 1, device=device, gradient_device=device)
    attacker = breaching_amd.prepare_attack(case.model, case.loss_fn, cfg, dict(device=device, dtype=torch.float))

    def call(dryrun):
        shared = [dict(gradients=list(d["gradients"]), buffers=d["buffers"], metadata=dict(d["metadata"])) for d in case.shared_data]
        torch.manual_seed(1234)  # the 32 starting points, drawn by rank 0 in the reference's order
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        rec, stats = attacker.reconstruct(case.server_payload, shared, {}, dryrun=dryrun)
        torch.cuda.synchronize(device)
        return rec, stats, time.perf_counter() - t0

    try:
        _, warm_stats, warm_s = call(dryrun=True)
        rec, stats, wall_s = call(dryrun=False)
    finally:
        attacker.close()
    execution = stats["execution"]
    ranks = max(pool_world, 1)
    histories = [stats[f"Trial_{t}_Val"] for t in range(num_trials)]
    modes = sorted(set(execution["trials"].values()))
    out = dict(
        config="BASELINE configs[3]: ResNet-18 ImageNet invertinggradients, restarts.num_trials=32, through attacker.reconstruct()",
        entry="TrialWorkerPool (single-process entry, workers.py)" if pool_world > 1 else "one process, one GPU",
        num_trials=num_trials, iterations_per_trial=iters, ranks=ranks, trials_per_rank=-(-num_trials // ranks),
        trials_in_flight_per_rank=min(4, -(-num_trials // ranks)),
        horizon_note=f"max_iterations shortened from the shipped 24 000 to {iters} (the step-lr milestones scale with it); every other "
                     "hyper-parameter as shipped, callback 1000",
        wall_s=round(wall_s, 3), trial_iterations_per_s=round(num_trials * iters / wall_s, 2),
        wall_includes="input shipping, prepare_attack, 32 random starts, the trial loops, rescoring every trial (:191-204), selection (:206-218)",
        timing_rank0=execution["timing"], pool=execution["pool"], pool_fallback=execution["pool_fallback"], oversubscribed=bool(oversubscribed),
        warmup_call_s=round(warm_s, 3), warmup_call="the same call with dryrun=True (one iteration per trial) first: pool start, MIOpen "
                                                     "solver look-ups and the stream calibration are paid there, not in wall_s",
        warmup_pool=warm_stats["execution"]["pool"],
        launch_modes=modes, histories_complete=bool(all(len(h) == iters for h in histories)),
        opt_value=stats["opt_value"], winner_final_loss_range=[round(min(h[-1] for h in histories), 6), round(max(h[-1] for h in histories), 6)],
        psnr_db_selected=round(psnr(rec["data"], case.true_user_data["data"], case.data_cfg), 4),
    )
    if ranks > 1 and committed_one_gpu:
        ref = committed_restarts32_one_gpu(iters, num_trials)
        if ref is not None:
            out["from_committed_profiles"] = dict(one_gpu=ref, strong_scaling_vs_one_gpu=round(ref["wall_s"] / wall_s, 3),
                                                  note="one-GPU wall of the same call from a committed run of this bench on another box (or hour); "
                                                       "the driver's own N = 1 line of the same round is the denominator proper")
    return out


def committed_restarts32_one_gpu(iters, num_trials):
    """The newest committed N = 1 line of this bench whose restarts32 leg ran the same horizon (profiles/r*_bench_driver_style*.json)."""
    import glob

    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_driver_style*.json")), reverse=True):
        try:
            with open(path) as f:
                leg = json.loads(f.read().strip().splitlines()[-1]).get("restarts32")
            if leg and leg.get("ranks") == 1 and leg.get("iterations_per_trial") == iters and leg.get("num_trials") == num_trials:
                return dict(wall_s=leg["wall_s"], trial_iterations_per_s=leg["trial_iterations_per_s"], file=os.path.basename(path))
        except Exception:
            continue
    return None


def restarts32_pool_subprocess(ranks, iters, num_trials, model_name, timeout):
    """The TrialWorkerPool shape of the leg in a process of its own (it must own the default process group): `python bench.py
    --restarts32-pool RANKS`, bounded; its one JSON line is returned (an error record on failure -- never fatal for the headline)."""
    import subprocess

    cmd = [sys.executable, os.path.abspath(__file__), "--restarts32-pool", str(ranks), "--restarts32-iters", str(iters),
           "--restarts32-trials", str(num_trials), "--model", model_name]
    try:
        env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_") and k not in ("OMP_NUM_THREADS",)}  # torchrun's: not this process's
        env["BREACH_HIP_POOL_START_TIMEOUT"] = os.environ.get("BREACH_HIP_POOL_START_TIMEOUT", str(int(timeout * 0.5)))
        proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
        for text in reversed(proc.stdout.splitlines()):
            if text.startswith("{"):
                return json.loads(text)
        return dict(error=f"no record (exit code {proc.returncode})", stderr=proc.stderr[-600:])
    except Exception as exc:
        return dict(error=repr(exc)[:400])


def dump_outputs(out_dir, trials):
    """`--dump-outputs DIR`: what the timed path handed back after its last step, per trial in flight on this rank -- the candidate
    (the tensor kernel B updates in place), the best copy kept by the loss commit, the objective of every step run so far (warm-up
    and timed) and [last objective, running minimum] -- as DIR/trial<t>_<name>.npy in float32.  `trials` = [(global trial index,
    FusedTrial)].  A few MB at the headline shape; the inputs are seeded, so two builds run with the same arguments can be compared
    file by file."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    written = 0
    for t, trial in trials:
        state = trial.read_state()
        arrays = dict(candidate=trial.candidates[0], best_candidate=trial.best()[0],
                      loss_history=trial.history[: min(trial.iterations, trial.max_iterations)],
                      objective=np.array([state["total"], state["minimum"]]))
        for name, value in arrays.items():
            host = value.detach().float().cpu().numpy() if hasattr(value, "detach") else value
            host = np.ascontiguousarray(host, dtype=np.float32)
            written += host.nbytes
            np.save(os.path.join(out_dir, f"trial{t}_{name}.npy"), host)
    assert written <= 64 * 2**20, f"--dump-outputs wrote {written} bytes, more than 64 MB"
    return written


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--full", action="store_true",
                   help="also run every leg beyond the headline figure (kernel events, roofline probes, live PMC, restarts32, selection "
                        "collectives, parity, GPU and CPU baselines); a plain run only sets up, warms up, times the steps and prints")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (float32); the "
                        "victim's convolutions then run on deterministic MIOpen solvers chosen without timing, so that two runs "
                        "compute the same outputs (several times slower per step than a plain run)")
    p.add_argument("--cpu-baseline-iters", type=int, default=80,
                   help="timed CPU iterations of the reference (or its port), ~10 s of host work (0 disables)")
    p.add_argument("--cpu-threads", type=int, default=0,
                   help="threads of the CPU baseline (0 = min(os.cpu_count(), 16): the measured optimum, profiles/r4_cpu_thread_sweep.json)")
    p.add_argument("--gm-cache-policy", default=None, metavar="FWD[,BWD]",
                   help="force kernel A's cache policy (0 auto / 1 plain / 2 non-temporal loads / 3 + non-temporal stores), forward[,backward]")
    p.add_argument("--gpu-torch-baseline-iters", type=int, default=60,
                   help="timed iterations of the PyTorch-ROCm port of the attack on the same GPU (0 disables); N = 1 only")
    p.add_argument("--no-live-pmc", action="store_true",
                   help="take roofline.traffic from the committed rocprofv3 --pmc passes instead of collecting it in this run (two bounded "
                        "rocprofv3 subprocesses over scripts/pmc_target.py after the timed region, ~30 s; N = 1 only)")
    p.add_argument("--no-parity", action="store_true", help="skip the teacher-forced parity evaluation against the reference fixture")
    p.add_argument("--no-hbm-resident", action="store_true", help="skip the BERT-base sized kernel-A timing (roofline.hbm_resident)")
    p.add_argument("--model", default="resnet18")
    p.add_argument("--no-kernel-timing", action="store_true")
    p.add_argument("--no-span-timing", action="store_true",
                   help="leave the device wall-clock span bookkeeping of kernel A off, as in the product path (it costs the "
                        "finalize kernel two dependent loads); the in-region span figure is then not reported")
    p.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay in the timed region")
    p.add_argument("--roofline-steps", type=int, default=40, help="eager iterations with per-launch HIP events")
    p.add_argument("--miopen-benchmark", action="store_true", help="torch.backends.cudnn.benchmark=True (MIOpen find mode)")
    p.add_argument("--channels-last", action="store_true", help="victim model and candidate in NHWC memory format")
    p.add_argument("--no-dry-collective", action="store_true",
                   help="N = 1 only: skip the one-rank RCCL run of the selection collectives (python -m breaching_amd.trials "
                        "--dry-collective, a bounded subprocess after the timed region)")
    p.add_argument("--restarts32-iters", type=int, default=1000,
                   help="iterations per trial of the restarts32 leg: BASELINE configs[3] (num_trials=32) through attacker.reconstruct(), "
                        "wall time incl. scoring and selection (0 disables); N = 1: 8 groups of 4 in flight on one GPU, N > 1: sharded")
    p.add_argument("--restarts32-trials", type=int, default=32)
    p.add_argument("--restarts32-pool", type=int, default=0, metavar="RANKS",
                   help="run ONLY the restarts32 leg through the single-process entry with a TrialWorkerPool of RANKS ranks (RCCL when "
                        "every rank has a GPU, gloo oversubscribed) and print its record; bench.py --gpus N runs this in a bounded "
                        "subprocess from rank 0 after the other ranks have left")
    p.add_argument("--trials-per-gpu", type=int, default=1,
                   help="independent restarts in flight per GPU on separate streams (BASELINE configs[3]: 32 trials on 8 GPUs = 4)")
    return p.parse_args(argv)


def main():
    args = parse_args()
    import torch
    import torch.distributed as dist

    private_db = False
    if args.dump_outputs:
        # The victim's convolutions run on MIOpen.  Its default solvers for this workload are not run-to-run reproducible (two eager runs
        # from a warm solver cache differ from the first iteration on: split-K weight-gradient kernels accumulate with atomics), and
        # hard-sign Adam turns a 1-ulp difference into another trajectory.  Deterministic solvers alone are not enough either: by default
        # MIOpen picks among them by timing whenever its user find-db has no entry, and reads earlier runs' entries otherwise, so the
        # choice depends on the home directory and on the clock.  A run whose outputs are meant for comparison therefore takes
        # deterministic solvers chosen by MIOpen's heuristics alone (FIND_MODE=FAST) against a user database of its own that starts
        # empty -- the same choice in every run of the same software on the same GPU -- at several times the plain run's time per step.
        # A plain run keeps the default solvers; `conv_solvers` in the line says which applied.  MIOpen reads these variables at its
        # first use, which comes later (build_case); explicit settings of the caller are kept.
        import atexit
        import shutil
        import tempfile

        torch.backends.cudnn.deterministic = True
        os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
        if "MIOPEN_USER_DB_PATH" not in os.environ:
            os.environ["MIOPEN_USER_DB_PATH"] = tempfile.mkdtemp(prefix="bench_miopen_userdb_")
            private_db = True
            atexit.register(shutil.rmtree, os.environ["MIOPEN_USER_DB_PATH"], True)

    import breaching_amd
    from breaching_amd import trials
    from breaching_amd.attacker import FusedTrial
    from breaching_amd.cases import build_case, initial_candidate

    if args.restarts32_pool > 1:  # the pool shape of the restarts32 leg alone (a process that owns its process group)
        for key in [k for k in os.environ if k.startswith("TORCHELASTIC_")] + ["WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK",
                                                                                "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE", "ROLE_NAME", "MASTER_ADDR", "MASTER_PORT"]:
            os.environ.pop(key, None)  # when started by a torch.distributed.run rank: this process is nobody's rank
        index = int(os.environ.get("BENCH_DEVICE_INDEX", "0"))
        torch.cuda.set_device(index)
        record = restarts32_leg(torch.device("cuda", index), args.model, args.restarts32_iters, args.restarts32_trials,
                                pool_world=args.restarts32_pool)
        record["device"] = device_record(torch.device("cuda", index))
        print(json.dumps(record), flush=True)
        return
    kernel_timing = args.full and not args.no_kernel_timing  # event pairs and the probes built on them: --full only
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # Bare `python bench.py --gpus N`: launch the N ranks ourselves, exactly the way the driver does, and pass the one
        # JSON line of rank 0 through.
        import subprocess

        from breaching_amd.workers import free_port

        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
               "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), *sys.argv[1:]]
        raise SystemExit(subprocess.run(cmd).returncode)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE={world}")
    if world > 1:
        # every rank is a first process on a fresh box: its own MIOpen user find-db, so that eight solver searches do not queue
        # on one sqlite lock (they all finish inside the untimed warm-up iterations; the barrier in front of the timed region
        # waits for the slowest)
        from breaching_amd.workers import isolate_miopen_user_db

        miopen_dir = isolate_miopen_user_db(rank)
    assert torch.cuda.is_available(), "bench.py needs a ROCm GPU"
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
    oversubscribed = world > torch.cuda.device_count()
    if oversubscribed:
        # Fewer GPUs than ranks (a 1-GPU box): ranks share devices round-robin and agree over gloo -- RCCL cannot put two
        # ranks on one device.  A functional check of the N > 1 path only; the line says so ("oversubscribed": true).
        local_rank = local_rank % torch.cuda.device_count()
        backend = "gloo"
    if "BENCH_DEVICE_INDEX" in os.environ:
        local_rank = int(os.environ["BENCH_DEVICE_INDEX"])
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import datetime

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
        limit = datetime.timedelta(seconds=float(os.environ.get("BREACH_HIP_COLLECTIVE_TIMEOUT", "600")))
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device, timeout=limit)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world, timeout=limit)
    if args.miopen_benchmark:
        torch.backends.cudnn.benchmark = True
    # Staged start (N > 1): rank 0 builds its trial and runs its warm-up first -- on a fresh box that is where MIOpen searches a solver
    # for every convolution configuration of the three autograd orders -- while the other ranks wait in front of their first
    # convolution; they then start from a COPY of rank 0's find-db: no eight concurrent searches (on one CPU, one sqlite lock) inside
    # the warm-up of the scaling run, and every rank runs the solvers rank 0 chose (equal speed, comparable results).
    # The release is a FILE FLAG with its own limit (BENCH_STAGED_START_TIMEOUT, default 300 s), not a collective: a slow or dead rank 0
    # must not hold seven ranks in a barrier until the collective timeout aborts the job -- on time-out they go ahead unseeded
    # (`staged_start.released` / `.seeded_files` per rank in the line).
    miopen_seeded, staged_released = None, None
    # (named after the launcher's PID -- the parent every rank of one torch.distributed.run launch shares -- so that a file left behind
    # by a crashed earlier launch on the same port cannot release this one's ranks early)
    staged_flag = os.path.join("/tmp", f"bench_staged_start_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}")
    if world > 1 and rank > 0:
        deadline = time.time() + float(os.environ.get("BENCH_STAGED_START_TIMEOUT", "300"))
        while not os.path.exists(staged_flag) and time.time() < deadline:
            time.sleep(0.05)
        staged_released = os.path.exists(staged_flag)
        from breaching_amd.workers import default_miopen_user_db, seed_miopen_user_db

        if staged_released and miopen_dir is not None and os.path.basename(miopen_dir).startswith("breach_hip_rank"):
            miopen_seeded = seed_miopen_user_db(os.path.join(default_miopen_user_db(), "breach_hip_rank0"), miopen_dir)

    # ---- workload --------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    case = build_case(args.model, "ImageNet", 1, device=device, gradient_device=device)
    # N = 1: a failed capture fails the bench.  N > 1 (a multi-rank run exists only on the driver's 8-GPU node and has never been
    # rehearsed): fall back to eager launches instead of losing the whole scaling run -- `launch_mode` / `graph_capture_error` say so
    overrides = [f"restarts.num_trials={world}", "impl.hip_graph=" + ("False" if args.no_graph else ("required" if world == 1 else "auto"))]
    if args.gm_cache_policy:
        parts = args.gm_cache_policy.split(",")
        overrides += [f"impl.gm_cache_policy={int(parts[0])}", f"impl.gm_cache_policy_bwd={int(parts[-1])}"]
    cfg = breaching_amd.get_attack_config("invertinggradients", overrides)
    setup = dict(device=device, dtype=torch.float)
    attacker = breaching_amd.prepare_attack(case.model, case.loss_fn, cfg, setup)
    rec_models, labels, stats = attacker.prepare_attack(case.server_payload, case.shared_data)
    attacker.objective.initialize(attacker.loss_fn, cfg.impl, None)
    for reg in attacker.regularizers:
        reg.initialize(rec_models, case.shared_data, labels)
    attacker.objective.prepare(rec_models, case.shared_data)  # pack the observed gradient (once, before the loop)
    for plan in attacker.objective._plans:
        plan.span_enabled = not args.no_span_timing  # must be set before the iteration is captured into the hipGraph
    x0 = initial_candidate(case.data_cfg, 1, trial=rank).to(device)
    if args.channels_last:
        for m in rec_models:
            m.to(memory_format=torch.channels_last)
        x0 = x0.contiguous(memory_format=torch.channels_last)
    x0 = x0.requires_grad_(True)
    # One trial: on the caller's stream, like `_fused_loop`.  Several in flight: every one on a side stream of its own, none on
    # the caller's (same layout as HipOptimizationAttacker._run_trial_group, see the measurement quoted there).
    main_stream = torch.cuda.current_stream(device)
    from breaching_amd.streams import calibration_report, side_streams

    # up to four trials: the product's measured choice of side streams (one hardware pipe each); more: plain pool streams
    side = side_streams(device, args.trials_per_gpu) if args.trials_per_gpu > 1 else []
    first_stream = side[0] if side else main_stream
    first_stream.wait_stream(main_stream)
    with torch.cuda.stream(first_stream):
        run = FusedTrial(attacker, [x0], labels, rec_models, case.shared_data)
    extra = []
    for j in range(1, args.trials_per_gpu):
        stream = side[j]
        stream.wait_stream(torch.cuda.current_stream(device))
        xj = initial_candidate(case.data_cfg, 1, trial=rank + world * j).to(device).requires_grad_(True)
        with torch.cuda.stream(stream):
            extra.append((stream, FusedTrial(attacker, [xj], labels, rec_models, case.shared_data)))

    def step_all():
        with torch.cuda.stream(first_stream):
            run.step()
        for stream, other in extra:
            with torch.cuda.stream(stream):
                other.step()
    n_elements = sum(p.numel() for p in rec_models[0].parameters())

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    if args.no_graph:
        run.disable_graph()
        for _, other in extra:
            other.disable_graph()
    # hipGraph capture happens after the third eager iteration; keep it out of the timed region even for tiny --warmup
    from breaching_amd.attacker import GRAPH_WARMUP_ITERATIONS

    warmup_steps = args.warmup if args.no_graph else max(args.warmup, GRAPH_WARMUP_ITERATIONS + 2)
    for _ in range(warmup_steps):
        step_all()
    if world > 1 and rank == 0:
        torch.cuda.synchronize(device)
        with open(staged_flag, "w") as f:  # releases the other ranks of the staged start (above)
            f.write("warm\n")
    plan = attacker.objective._plan
    timed_with_events = plan is not None and kernel_timing and run.graph is None
    if timed_with_events:
        plan.enable_timing()  # eager timed region: the events ride inside it
    if plan is not None:
        plan.span_accum.zero_()  # device-side wall-clock spans of kernel A forward, accumulated by the finalize kernel
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step_all()
    barrier()
    elapsed = time.perf_counter() - t0
    span_us, span_launches = plan.forward_span_us() if plan is not None else (None, 0)
    per_rank_ms = None
    if world > 1:
        mine = torch.tensor([elapsed], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        everyone = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(everyone, mine)  # every rank's own wall time of the same K steps: the skew shows a straggler GPU / rank
        per_rank_ms = [round(float(v.item()) / args.steps * 1e3, 4) for v in everyone]
        staged = [None] * world
        dist.all_gather_object(staged, dict(rank=rank, released=staged_released, seeded_files=miopen_seeded))
        if rank == 0:
            try:
                os.remove(staged_flag)
            except OSError:
                pass
        t = mine.clone()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    mode = "hipGraph replay" if run.graph is not None else "eager launches"
    graph_failed = run.graph_failed
    if args.dump_outputs:  # before any later leg steps the trials on
        dump_outputs(args.dump_outputs, [(rank, run)] + [(rank + world * j, other) for j, (_, other) in enumerate(extra, 1)])

    # A replayed graph cannot carry host-visible event pairs, so when the timed region ran as graph replays the same
    # iteration body is continued eagerly for a few more steps with a HIP event pair around every kernel-A launch.
    eager_ms = None
    if plan is not None and kernel_timing and not timed_with_events:
        run.disable_graph()
        with torch.cuda.stream(first_stream):
            for _ in range(3):
                run.step()
        plan.enable_timing()
        barrier()
        te = time.perf_counter()
        with torch.cuda.stream(first_stream):
            for _ in range(args.roofline_steps):
                run.step()
        barrier()
        eager_ms = (time.perf_counter() - te) / max(args.roofline_steps, 1) * 1e3

    # ---- kernel timing (HIP events recorded on the launch stream during the timed region) -----------------------------
    roofline = None
    kernels = {}
    if plan is not None and plan.timers is not None:
        measured = plan.drain_timers()
        for key, bytes_per in (("fwd", 2 * n_elements * 4), ("bwd", 3 * n_elements * 4), ("fin", None)):
            us = sorted(measured.get(key, []))
            if us:
                avg_us = sum(us) / len(us)
                kernels[key] = dict(avg_us=avg_us, median_us=us[len(us) // 2], min_us=us[0], launches=len(us))
                if bytes_per is not None:
                    kernels[key].update(algorithmic_bytes=bytes_per, achieved_GBs=bytes_per / (avg_us * 1e-6) / 1e9)
        if "fin" in kernels:
            kernels["fin"]["note"] = ("gm_finalize_kernel (one workgroup, <= 512 rows): start/stop events of "
                                      "hipExtLaunchKernelGGL, like the forward launch")
    # Kernel A forward: average launch duration from HIP events (hipExtLaunchKernelGGL start/stop events = the dispatch's
    # own begin/end timestamps, the quantity rocprofv3 reports).  A replayed graph cannot carry events, so when the timed
    # region ran as graph replays they come from the eager continuation right after it, and the device wall-clock span
    # (first workgroup in -> last workgroup out) of every launch INSIDE the timed region is reported next to them.
    fwd_bytes = 2 * n_elements * 4
    traffic_files = []
    if "fwd" in kernels:
        k = kernels["fwd"]
        roofline = dict(bound="hbm", kernel="gm_fwd_kernel<cosine>", achieved=round(k["achieved_GBs"], 1), peak=HBM_PEAK_GBS,
                        unit="GB/s", frac=round(k["achieved_GBs"] / HBM_PEAK_GBS, 4),
                        traffic=pmc_traffic_bytes("gm_fwd_kernel", traffic_files),
                        traffic_source="committed rocprofv3 --pmc passes of the same kernel at the same list size (scripts/pmc_target.py; not "
                                       "collected in this run): " + ", ".join(traffic_files),
                        avg_launch_us=round(k["avg_us"], 2), launches=k["launches"], algorithmic_bytes=fwd_bytes,
                        measured="HIP start/stop events of hipExtLaunchKernelGGL on the launch stream, " +
                                 ("inside the timed region" if timed_with_events else
                                  f"{args.roofline_steps} eager iterations continuing the timed graph-replay region"),
                        timed_region_span_us=None if not span_us else round(span_us, 2),
                        timed_region_span_launches=span_launches,
                        timed_region_span_GBs=None if not span_us else round(fwd_bytes / (span_us * 1e-6) / 1e9, 1),
                        timed_region_span_note="device wall clock, first workgroup in -> last workgroup out of every forward "
                                               "launch INSIDE the timed graph-replay region (excludes dispatch latency)",
                        # both gradient lists (2 x 46.8 MB for ResNet-18) fit the 256 MiB Infinity Cache and `r` was just
                        # written by autograd: the achieved rate is partly a cache figure, not pure HBM
                        infinity_cache_resident=bool(fwd_bytes <= 256 * 2 ** 20))
        replay_us, replay_file = committed_replay_duration("gm_fwd_kernel<0")
        if replay_us and args.model == "resnet18":  # NOT measured in this run: kept apart, under a name that says so
            roofline["from_committed_profiles"] = dict(in_graph_replay=dict(
                avg_launch_us=replay_us, frac=round(fwd_bytes / replay_us / 1e3 / HBM_PEAK_GBS, 4),
                source=f"rocprofv3 kernel trace of this command, committed ({replay_file}): the timed region replays a hipGraph, where "
                       "event pairs cannot ride; the events above time the same kernel on eager launches"))
        if "fin" in kernels:  # the whole forward stage: reduction + one-workgroup finalize
            stage_us = k["avg_us"] + kernels["fin"]["avg_us"]
            roofline.update(stage_us=round(stage_us, 2), stage_GBs=round(fwd_bytes / (stage_us * 1e-6) / 1e9, 1),
                            stage_frac=round(fwd_bytes / (stage_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4))
    elif span_us:
        achieved = fwd_bytes / (span_us * 1e-6) / 1e9
        roofline = dict(bound="hbm", kernel="gm_fwd_kernel<cosine>", achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=round(achieved / HBM_PEAK_GBS, 4), traffic=pmc_traffic_bytes("gm_fwd_kernel"),
                        avg_launch_us=round(span_us, 2), launches=span_launches, algorithmic_bytes=fwd_bytes,
                        measured="device wall clock (first workgroup in -> last workgroup out) of every launch in the timed region")
    if roofline is not None and rank == 0 and world == 1 and not args.no_hbm_resident and kernel_timing:
        try:
            with torch.cuda.stream(first_stream):
                roofline["hbm_resident"] = hbm_resident_leg(device)
        except Exception as exc:  # e.g. out of memory next to another tenant: reported, never fatal for the headline value
            roofline["hbm_resident"] = dict(error=repr(exc))
    if roofline is not None and "fwd" in kernels and rank == 0 and world == 1 and kernel_timing:
        try:
            with torch.cuda.stream(first_stream):
                roofline["ceiling"] = read_ceiling_leg(device, n_elements, kernels["fwd"]["avg_us"])
            if "us" in roofline["ceiling"]:
                roofline["frac_of_ceiling"] = round(roofline["ceiling"]["us"] / kernels["fwd"]["avg_us"], 4)
        except Exception as exc:  # the diagnostic library is not part of the product: its absence never fails the bench
            roofline["ceiling"] = dict(error=repr(exc)[:300])
    live = None
    if roofline is not None and rank == 0 and world == 1 and not args.no_live_pmc and kernel_timing and args.model in ("resnet18", "resnet50"):
        live = pmc_traffic_live(args.model)
        if live and "gm_fwd_kernel" in live:
            roofline["traffic"] = live["gm_fwd_kernel"]
            roofline["traffic_source"] = ("collected in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, separate bounded passes over "
                                          "scripts/pmc_target.py (kernel A alone at this list size), FETCH_SIZE x 2 + WRITE_SIZE")
            roofline["traffic_over_algorithmic"] = round(live["gm_fwd_kernel"] / fwd_bytes, 4)
    if "bwd" in kernels:
        kernels["bwd"]["traffic"] = live["gm_bwd_kernel"] if live and "gm_bwd_kernel" in live else pmc_traffic_bytes("gm_bwd_kernel")
        kernels["bwd"]["frac_of_hbm_peak"] = round(kernels["bwd"]["achieved_GBs"] / HBM_PEAK_GBS, 4)

    # ---- trial selection: the one collective of the multi-GPU path --------------------------------------------------
    select_ms = score_ms = None
    state = run.read_state()
    if world > 1 and args.full:
        torch.cuda.synchronize(device)
        ts = time.perf_counter()
        shard = trials.TrialShard.current(world)
        best = run.best()[0]
        # scored exactly as `reconstruct` scores a finished trial (optimization_based_attack.py:191-204), not by the running minimum
        score = attacker._score_trial(best, labels, rec_models, case.shared_data)
        torch.cuda.synchronize(device)
        tm = time.perf_counter()
        value, _ = shard.select({rank: best}, {rank: score}, stats, device, gather_stats=False)  # all-reduce + broadcast
        torch.cuda.synchronize(device)
        score_ms, select_ms = (tm - ts) * 1e3, (time.perf_counter() - tm) * 1e3

    # ---- BASELINE configs[3] through the product entry, one GPU: 8 groups of 4 trials in flight (after the timed region) ------
    restarts32 = None
    if args.full and world == 1 and args.restarts32_iters > 0 and args.model == "resnet18":
        try:
            restarts32 = restarts32_leg(device, args.model, args.restarts32_iters, args.restarts32_trials)
        except Exception as exc:  # reported, never fatal for the headline value
            restarts32 = dict(error=repr(exc)[:400])

    # ---- N = 1: the selection collectives through a one-rank RCCL communicator (bounded subprocess, off the timed region) ---
    rccl_dry_run = None
    if args.full and world == 1 and not args.no_dry_collective:
        import subprocess

        try:
            proc = subprocess.run([sys.executable, "-m", "breaching_amd.trials", "--dry-collective", "nccl", str(device)], cwd=ROOT,
                                  capture_output=True, text=True, timeout=150)
            rccl_dry_run = trials.parse_dry_collective(proc.stdout) if proc.returncode == 0 else None
            if rccl_dry_run is None:
                rccl_dry_run = dict(ok=False, returncode=proc.returncode, stdout=proc.stdout[-300:], stderr=proc.stderr[-400:])
        except Exception as exc:  # a timeout included: reported, never fatal for the measurement
            rccl_dry_run = dict(ok=False, error=repr(exc))

    # ---- parity of the timed configuration + the same-GPU PyTorch baseline (rank 0, N == 1 only; after the timed region) -----
    parity = gpu_torch_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_parity:
        try:
            parity = parity_leg(device, args.model)
        except Exception as exc:
            parity = dict(error=repr(exc)[:300])
    if args.full and rank == 0 and world == 1 and args.gpu_torch_baseline_iters > 0:
        try:
            gpu_torch_baseline = gpu_torch_baseline_leg(device, args.model, args.gpu_torch_baseline_iters)
        except Exception as exc:
            gpu_torch_baseline = dict(error=repr(exc)[:300])

    # ---- CPU baseline (rank 0, N == 1 only) ---------------------------------------------------------------------------
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and args.cpu_baseline_iters > 0:
        cpu_baseline = cpu_baseline_leg(args.model, args.cpu_baseline_iters, args.cpu_threads)

    if world > 1:
        dist.destroy_process_group()  # ranks > 0 are done: they leave, and with them their hold on the other GPUs
    if args.full and rank == 0 and world > 1 and args.restarts32_iters > 0 and args.model == "resnet18":
        # BASELINE configs[3] as north_star states it: the 32 restarts over the N GPUs through the product's single-process entry
        # (TrialWorkerPool over RCCL), in a bounded process of its own -- a failure or a time-out is a record, never a lost line
        restarts32 = restarts32_pool_subprocess(world, args.restarts32_iters, args.restarts32_trials, args.model, timeout=900)
    if rank == 0:
        line = {
            "metric": "attack iters/sec, ResNet-18 ImageNet invertinggradients; PSNR vs ref",
            "value": round(world * args.trials_per_gpu * args.steps / elapsed, 3),
            "unit": "attack iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": warmup_steps,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),  # one step of every trial in flight
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{args.model} (1000 classes, random init) 1x3x224x224, attack=invertinggradients "
                                   "(cosine + TV 0.2, hard-sign Adam, boxed), " +
                                   ("one trial per GPU" if args.trials_per_gpu == 1 else
                                    f"{args.trials_per_gpu} independent trials in flight per GPU (separate streams)"),
                       "gradient_list_elements": n_elements, "trials": world * args.trials_per_gpu,
                       "trials_in_flight_per_gpu": args.trials_per_gpu, "parallelism": f"trial-parallel x{world}"},
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
            "gpu_torch_baseline": gpu_torch_baseline,
            "parity": parity,
            "kernels": kernels,
            "launch_mode": mode,
            "eager_ms_per_step": None if eager_ms is None else round(eager_ms, 4),
            "graph_capture_error": graph_failed,
            "final_objective": state["total"],
            "trial_streams": calibration_report(device) if args.trials_per_gpu > 1 else None,
            "per_rank_ms_per_step": per_rank_ms,
            "rank_skew": None if not per_rank_ms else round(max(per_rank_ms) / min(per_rank_ms), 4),
            "select_ms": select_ms,
            "score_ms": score_ms,
            "restarts32": restarts32,
            "rccl_dry_run": rccl_dry_run,
            "collective_backend": backend if world > 1 else None,
            "oversubscribed": bool(oversubscribed),
            "device": device_record(device, clocks=args.full),
            "conv_solvers": (dict(deterministic=True, find_mode=os.environ.get("MIOPEN_FIND_MODE"), user_db="private to this run" if private_db else os.environ.get("MIOPEN_USER_DB_PATH"))
                             if args.dump_outputs else dict(deterministic=False, find_mode="MIOpen default", user_db="MIOpen default")),
            "staged_start": None if world == 1 else dict(how="rank 0 warms up first; ranks > 0 wait for its file flag (bounded) and start from a copy "
                                                             "of its MIOpen find-db", ranks=staged[1:]),
        }
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

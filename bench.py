#!/usr/bin/env python3
"""Headline benchmark: synthesised 256x256 vehicle crops / second on N MI355X (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W          (starts its own N ranks when N > 1)
    python bench.py ... --full                             (+ every secondary measurement, see below)
    python bench.py ... --dump-outputs DIR                 (+ the last timed step's outputs as DIR/<name>.npy)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One *step* = one pass of the hot path over one batch of synthetic crops per rank:
hourglass (+argmax) -> ICN -> VUnet first-frame (enc_up, enc_down, dec_up, dec_down) -> uint8
quantisation [+ EdgeGenerator + InpaintGenerator with --inpaint], then (N > 1) the gather of the
rendered uint8 crops to rank 0 over RCCL.  The default workload is BASELINE.json configs[1]:
batch 32 of 256x256 crops per GPU.  Tensors are fp32 (the reference's dtype) everywhere.

A plain run does only what the headline needs: set-up, the DVFS settle and W warm-up steps, K timed steps of the
f16x3 leg, the outputs of the last timed step written with --dump-outputs DIR, and the result line.  Everything else
below (the f32 and bf16 legs, the roofline pass, power sampling, the CPU baseline and the secondary figures) runs only
with --full; the --no-* options switch parts of --full off.

Precision legs.  The conv contraction exists in two arithmetics and a --full run times both, each with the full
protocol (W warm-up steps, K timed steps between barrier + synchronize, max over ranks, roofline pass):
  f32   : exact fp32 MFMA (v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf chain) - the reference's arithmetic.
  f16x3 : fp32 operands split into scaled fp16 pairs, three fp16 MFMA products, fp32 accumulation
          (csrc/conv_kernel_h3.h).  Error vs fp64 within 1.3x of the f32 kernel's over operand scales 1e-3..1e2
          (observed 0.96-1.27x; tests/test_gpu_ops.py::test_f16x3_scale_sweep asserts 2x; profiles/r02_parity.json);
          operands outside the split's
          range raise a device-side status word and the pass is redone in f32 (never a silent clamp) - the
          benchmark checks that word once after the timed steps and refuses the leg if it was raised.
The headline `value` is the f16x3 leg (fp32-class accuracy, defended by the tests above); "precision_legs" carries
every leg that ran in the same line.  --precision chooses the legs (default: f16x3, or all three with --full).

Inputs and weights are synthetic (no datasets / checkpoints in this environment) and resident in HBM before
the timed region; VUnet's sampler noise is drawn on the CPU generator inside the step, as the reference does.
Weak scaling: each rank processes its own batch (vehicles are independent); --vehicles V is the strong-scaling
mode of BASELINE configs[3] (one frame's V vehicles sharded over the ranks, e.g. --gpus 8 --vehicles 64).

Extra fields of a --full run: "roofline" (conv kernels: algorithmic FLOPs of SURVEY.md §8d - and the FLOPs as launched - divided
by the kernels' HIP-event time on the launch stream, measured live in a second pass of the same K steps),
"cpu_baseline" (the CPU oracle = a port of the reference's torch graph, timed on this host's cores on a bounded
sample of the same workload, the whole leg capped at 60 s; N=1, rank 0 only), "ssim_vs_cpu_ref" / "kp_idx_exact" (quality of the GPU path on
that very sample), "clip_mode" (secondary figure: 8 vehicles x 6 frames) and "frame_mode" (secondary figure: the
chained per-frame driver run_frame, 8 vehicles on a 720 x 1280 frame).
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# algorithmic conv FLOPs per crop at 256x256 (2*MAC, measured on the reference)
GFLOP_PER_CROP = {"hg": 17.95, "icn": 130.12, "vunet_first": 76.27, "edge": 96.13, "inpaint": 97.37}
PEAK_F32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md, v_mfma_f32_32x32x2_f32 dense peak
PEAK_F16_MFMA_TFLOPS = 2500.0       # MI355X_MICROARCH.md, dense fp16/bf16 MFMA peak (no sparsity)
DTYPE = {"f32": "f32",
         "bf16": "f32 tensors; halo-kernel conv layers of ICN / VUnet / EdgeConnect contract in single-pass bf16 MFMA (f32 accumulate), "
                 "remaining layers and the whole hourglass in f16x3 (BASELINE configs[4]'s bf16 path; SSIM >= 0.999, keypoints exact)",
         "f16x3": "f32 tensors; conv contraction as 3 fp16 MFMA products of scaled (hi, lo) operand splits, f32 accumulate "
                  "(error vs fp64 <= 1.3x the exact-f32 MFMA kernel's: observed 0.96-1.27x over 12 operand scales x 5 layers; "
                  "range-guarded; exact-f32 leg in precision_legs)"}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--vehicles", type=int, default=0,
                    help="strong scaling (BASELINE configs[3], e.g. 64): this many vehicles in total, sharded over the "
                         "ranks (default: --batch per rank, weak scaling)")
    ap.add_argument("--settle-s", type=float, default=0.6, help="seconds of untimed steps before the warm-up steps (DVFS settle)")
    ap.add_argument("--batch", type=int, default=32, help="crops per GPU per step")
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--inpaint", action="store_true", help="BASELINE configs[2]: add EdgeConnect")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU-baseline leg")
    ap.add_argument("--cpu-sample", type=int, default=8, help="crops in the CPU baseline sample (--full)")
    ap.add_argument("--no-clip", action="store_true", help="--full without the secondary figures (clip / frame mode, configs[0])")
    ap.add_argument("--no-prof", action="store_true", help="--full without the roofline leg (second pass with per-launch HIP events)")
    ap.add_argument("--broadcast-weights", dest="broadcast_weights", action="store_true", default=True,
                    help="N > 1 (default): only rank 0 builds the checkpoints, the others receive them through "
                         "pipeline.broadcast_state_dicts (RCCL broadcast of one flat blob per network) - what a real "
                         "checkpoint read on rank 0 needs")
    ap.add_argument("--no-broadcast-weights", dest="broadcast_weights", action="store_false",
                    help="N > 1: every rank rebuilds the synthetic weights from the seed instead (no start-up collective)")
    ap.add_argument("--replay", action="store_true",
                    help="issue each pass as ONE recorded-plan replay (fusg_plan) instead of ~370 launches from Python: "
                         "matters at small --batch, where the interpreter bounds the pass")
    ap.add_argument("--precision", choices=["f16x3", "f32", "bf16", "both", "all"], default=None,
                    help="which precision legs to time (default f16x3, all three with --full; the headline is f16x3 when it "
                         "ran, bf16 is the reduced-precision path of BASELINE configs[4] and never the headline of an fp32 "
                         "configuration)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement: the f32 and bf16 legs, the roofline pass, power sampling, the "
                         "CPU baseline, clip / frame mode and configs[0] (a plain run times the headline leg only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the headline leg's last timed step (rank 0) as "
                         "DIR/<name>.npy, float32 (int32 indices as float64), at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_BUDGET_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 0


def dump_outputs(outputs, path, budget=DUMP_BUDGET_BYTES):
    """Write host copies of one step's outputs (name -> CPU tensor, all with the crops as leading dimension) as
    path/<name>.npy: integer indices as float64 (exact), everything else as float32.  When the arrays together exceed
    `budget` bytes, every array keeps the same fixed, seeded sample of crops (rows of the leading dimension, in order).
    Returns {name: shape written}."""
    import numpy as np
    arrs = {}
    for k, v in sorted(outputs.items()):
        a = v.numpy()
        arrs[k] = a.astype(np.float64 if a.dtype in (np.int32, np.int64, np.float64) else np.float32)
    total = sum(a.nbytes for a in arrs.values())
    rows = min((a.shape[0] for a in arrs.values()), default=0)
    if total > budget and rows > 1:
        keep = max(1, rows * budget // total)
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(rows, size=keep, replace=False))
        arrs = {k: a[idx] for k, a in arrs.items()}
    os.makedirs(path, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a))
    return {k: list(a.shape) for k, a in arrs.items()}


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start N copies of this script, one per GPU, as CHILD processes
    (this parent has not touched HIP and never does - an exec from a GPU-initialised process is forbidden on the
    pool), wait for them and return the worst exit status.  Rank 0's JSON line goes to the inherited stdout."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", str(port)),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    # Poll instead of waiting rank by rank: when one rank dies early (bad device, import error, OOM) the survivors
    # would sit in init_process_group / barrier / gather until the collective's own timeout (10 minutes and more)
    # and hold their GPUs; the launcher ends them as soon as the first failure is seen and returns that status.
    rc = 0
    while True:
        alive = 0
        for p in procs:
            code = p.poll()
            if code is None:
                alive += 1
            elif code != 0 and rc == 0:
                rc = code
        if rc or not alive:
            break
        time.sleep(0.05)
    if rc:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        t_end = time.time() + 10
        for p in procs:
            try:
                p.wait(timeout=max(0.1, t_end - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    return rc


class PowerSampler:
    """Socket power / shader clock of the card under test, sampled from sysfs hwmon while the timed steps run.
    The big layers run at the 1400 W board limit, so this is part of reading the number."""

    def __init__(self, pci_bdf=None):
        import glob
        self.p = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/power1_input") +
                        glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/power1_average"))
        if pci_bdf:                                 # keep only the card under test (PCI address match)
            mine = [x for x in self.p if pci_bdf in os.path.realpath(x.split("/hwmon/")[0])]
            if mine:
                self.p = mine[:1]
        self.f = [os.path.join(os.path.dirname(x), "freq1_input") for x in self.p]
        self.samples, self._stop, self._th = [], False, None
        self.idle = [self._read(x) for x in self.p]

    @staticmethod
    def _read(path):
        try:
            return int(open(path).read().strip())
        except (OSError, ValueError):
            return 0

    def start(self):
        import threading

        def loop():
            while not self._stop:
                self.samples.append(([self._read(x) for x in self.p], [self._read(x) for x in self.f]))
                time.sleep(0.01)

        if self.p:
            self._th = threading.Thread(target=loop, daemon=True)
            self._th.start()

    def stop(self):
        self._stop = True
        if self._th is None:
            return None
        self._th.join()
        if not self.samples:
            return None
        self.samples = self.samples[len(self.samples) // 2:]                   # the sensor lags by up to ~1 s: steady half
        n = len(self.samples)
        avg = [sum(s[0][i] for s in self.samples) / n for i in range(len(self.p))]
        k = max(range(len(self.p)), key=lambda i: avg[i] - self.idle[i])       # the card whose power rose
        return {"avg_w": round(avg[k] / 1e6, 1), "max_w": round(max(s[0][k] for s in self.samples) / 1e6, 1),
                "sclk_mhz": round(sum(s[1][k] for s in self.samples) / n / 1e6), "samples": n,
                "source": "sysfs hwmon power1/freq1 of the card under test, 10 ms period, second half of the headline leg"}


def cpu_model() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


CPU_SWEEP_THREADS = (8, 16, 32, 64)     # never "all CPUs": 256 threads ran at 0.0115 crops/s on the driver's box (round 2)
CPU_SWEEP_POINT_S = 10.0                # a sweep point that needs longer than this is abandoned (and so are the wider ones)
CPU_LEG_BUDGET_S = 60.0                 # the whole CPU-baseline leg


def cpu_sweep_points(ncpu: int, default_threads: int):
    """Thread counts the CPU-baseline sweep tries on a host with `ncpu` usable CPUs."""
    return sorted(t for t in CPU_SWEEP_THREADS if t <= ncpu) or [min(ncpu, max(1, default_threads))]


def cpu_baseline_leg(args, batch, pipe, torch):
    """the CPU oracle (a port of the reference's torch graph) on this host's cores, bounded to
    CPU_LEG_BUDGET_S.  The thread count is chosen ON THE SAMPLE THAT IS REPORTED (--cpu-sample crops as one batch):
    every count of {8, 16, 32, 64} the host has gets a 1-crop warm-up and one timed pass over the sample (a point
    that overruns CPU_SWEEP_POINT_S is abandoned and ends the sweep); the best count then gets up to two more passes
    (as many as fit the budget) and the fastest pass of that count is reported, with per-network seconds.  Returns
    (cpu_baseline dict, quality dict of the GPU path on the same sample and noise seed)."""
    import numpy as np

    import oracle
    from future_urban_scene_generation_amd.pipeline import load_schema
    from future_urban_scene_generation_amd.synth import synth_state_dict
    t_leg = time.perf_counter()
    ns = max(1, min(args.cpu_sample, args.batch))
    sds = {n: synth_state_dict(n, load_schema(n), 0)
           for n in (("hg", "icn", "vunet") + (("edge", "inpaint") if args.inpaint else ()))}
    cpu_batch = {k: v[:ns].cpu() for k, v in batch.items()}
    one = {k: v[:1] for k, v in cpu_batch.items()}
    ncpu = os.cpu_count() or 1
    try:
        ncpu = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    default_threads = torch.get_num_threads()
    points = cpu_sweep_points(ncpu, default_threads)
    sweep, runs = {}, {}                                # threads -> crops/s ; threads -> (seconds, per-net seconds, outputs)

    def timed_pass(deadline=None):
        secs = {}
        torch.manual_seed(77)
        t1 = time.perf_counter()
        ref = oracle.crop_pass(sds, cpu_batch, args.inpaint, seconds=secs, deadline=deadline)
        return time.perf_counter() - t1, secs, ref

    for nt in points:
        torch.set_num_threads(nt)
        dl = time.perf_counter() + CPU_SWEEP_POINT_S
        try:
            oracle.crop_pass(sds, one, args.inpaint, deadline=dl)          # warm-up (thread pool, oneDNN primitives)
            runs[nt] = timed_pass(dl)
            sweep[nt] = round(ns / runs[nt][0], 4)
        except TimeoutError:
            sweep[nt] = None                    # abandoned; wider points were slower still wherever this was seen
            break
        if time.perf_counter() - t_leg > CPU_LEG_BUDGET_S * 0.6:
            break
    if not runs:                                # even the narrowest point overran: time it without a deadline, once
        torch.set_num_threads(points[0])
        runs[points[0]] = timed_pass()
        sweep[points[0]] = round(ns / runs[points[0]][0], 4)
    best_nt = min(runs, key=lambda k: runs[k][0])
    best, best_secs, ref = runs[best_nt]
    passes = 1
    torch.set_num_threads(best_nt)
    while passes < 3 and time.perf_counter() - t_leg + best < CPU_LEG_BUDGET_S:
        dt, secs, r = timed_pass()
        passes += 1
        if dt < best:
            best, best_secs, ref = dt, secs, r
    torch.set_num_threads(default_threads)
    base = {"value": round(ns / best, 4), "unit": "crops/s", "cores": best_nt, "kind": "port",
            "cpu": cpu_model(), "host_cpus": ncpu, "batch": ns,
            "sample": f"{ns} crops of the same workload as ONE batch of {ns} (the GPU leg runs batch {args.batch}); the thread count "
                      f"is the best of a sweep over {list(points)} threads on this very sample (1-crop warm-up + one timed pass "
                      f"per point), then best of {passes} pass(es) at that count",
            "thread_sweep_crops_per_s": {str(k): v for k, v in sweep.items()},
            "seconds_per_net": {k: round(v, 3) for k, v in best_secs.items()},
            "leg_seconds": round(time.perf_counter() - t_leg, 1)}
    torch.manual_seed(77)
    got = pipe.run({k: v[:ns] for k, v in batch.items()})
    quality = {"ssim_vs_cpu_ref": round(min(oracle.ssim(got["icn_u8"].cpu().numpy(), ref["icn_u8"]),
                                            oracle.ssim(got["vunet_u8"].cpu().numpy(), ref["vunet_u8"])), 6),
               "kp_idx_exact": bool(np.array_equal(got["kp_idx"].cpu().numpy(), ref["kp_idx"]))}
    return base, quality


def vunet_forward_leg(args, pipe, torch, with_cpu=True, threads=None):
    """BASELINE configs[0] ("single 256x256 crop, vunet.models forward only, --device cpu"): the latency of ONE
    `Vunet_fix_res.forward(y_tilde, x)` call at batch 1 - the drop-in module called eagerly (what run_test.py would do),
    the pipeline's form of the same call (shape encoder on its side stream) eagerly and as a recorded-plan replay -
    beside the CPU oracle's seconds for the same call on this host (default torch thread count; best of 3)."""
    import oracle
    from future_urban_scene_generation_amd.pipeline import load_schema, synth_batch
    from future_urban_scene_generation_amd.synth import synth_state_dict
    dev = pipe.device
    b1 = synth_batch(1, args.res, dev, seed=5)
    b1 = {"vu_x": b1["vu_x"], "vu_y": b1["vu_y"]}
    vu = pipe.vunet
    vu.set_vehicle_seeds(None)

    def lat(fn, n=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):                              # latency: every call waits for its result
            t1 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t1)
        ts.sort()
        return ts[len(ts) // 2] * 1e3

    out = {"workload": "Vunet_fix_res.forward(y_tilde [1,3,%d,%d], x [1,6,%d,%d]), one call at a time" % ((args.res,) * 4),
           "ms_module_forward_eager": round(lat(lambda: vu.forward(b1["vu_y"], b1["vu_x"])), 3),
           "ms_pipeline_eager": round(lat(lambda: pipe.vunet_forward(b1, check="async")), 3)}
    pipe.finish()
    cp = pipe.compile(b1, None, fn=pipe._vunet_forward)
    out["ms_pipeline_replay"] = round(lat(lambda: cp.run(b1, check="async")), 3)
    out["range_status_raised"] = bool(pipe.finish())
    if with_cpu:
        sd = synth_state_dict("vunet", load_schema("vunet"), 0)
        y, x = b1["vu_y"].cpu(), b1["vu_x"].cpu()
        default_threads = torch.get_num_threads()
        if threads:
            torch.set_num_threads(int(threads))              # the count the cpu_baseline sweep found best on this host
        oracle.vunet_forward(sd, y, x)
        best = None
        for _ in range(3):
            torch.manual_seed(5)
            t1 = time.perf_counter()
            ref = oracle.vunet_forward(sd, y, x)[0]
            dt = time.perf_counter() - t1
            best = dt if best is None or dt < best else best
        torch.manual_seed(5)
        got = pipe.vunet_forward(b1)["vunet_u8"].cpu().numpy()
        out["cpu_port_ms"] = round(best * 1e3, 1)
        out["cpu_threads"] = torch.get_num_threads()
        torch.set_num_threads(default_threads)
        out["ssim_vs_cpu_ref"] = round(float(oracle.ssim(got, oracle.to_image_u8(ref))), 6)
    return out


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: be the launcher.  Nothing above this line (and nothing in this branch) touches HIP.
        raise SystemExit(spawn_ranks(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("FUSG_BENCH_DRYRUN"):             # tests/test_bench_cpu.py: what each started rank was given
        print(json.dumps({"rank": rank, "local_rank": local_rank, "world": world, "gpus": args.gpus,
                          "master": "%s:%s" % (os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"))}), flush=True)
        # rehearsal of a rank that dies early while the others wait at a collective (tests/test_bench_cpu.py)
        if os.environ.get("FUSG_BENCH_DRYRUN_FAIL_RANK") == str(rank):
            raise SystemExit(3)
        time.sleep(float(os.environ.get("FUSG_BENCH_DRYRUN_SLEEP", "0")))
        return

    import torch
    import torch.distributed as dist

    # FUSG_DIST_FORCE=1 (test hook, tests/test_bench_gpu.py): treat ONE rank as a multi-rank job - the process group is initialised and every
    # collective of the multi-rank path (weight broadcast, crop gather, barrier, all-reduce of the timings) goes through RCCL with a
    # communicator of one rank: what a box with a single card can execute of the RCCL path
    multi = world > 1 or os.environ.get("FUSG_DIST_FORCE") == "1"
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback for the product path)")
    backend = os.environ.get("FUSG_DIST_BACKEND", "nccl")
    if backend != "nccl":                               # rehearsal: ranks share the cards that exist
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if multi:
        # RCCL ("nccl" on ROCm).  FUSG_DIST_BACKEND=gloo rehearses the multi-rank code path where the ranks have
        # to share one card (development boxes): the gathers are then staged through host memory.
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    coll_dev = dev if (world == 1 or backend == "nccl") else "cpu"

    from future_urban_scene_generation_amd import ops
    from future_urban_scene_generation_amd.pipeline import VehiclePipeline, gather_in_order, shard_range, synth_batch

    torch.set_grad_enabled(False)
    if world > 1:                                       # (not `multi`: one rank keeps the whole host)
        # N ranks share one host: each draws its VUnet noise with torch.randn on the CPU and issues ~370 launches
        # per pass - without a cap every rank starts a thread pool as wide as the machine
        try:
            ncpu = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            ncpu = os.cpu_count() or 1
        torch.set_num_threads(max(1, min(16, ncpu // world)))
    sds, bcast_ms = None, None
    if args.broadcast_weights and multi:
        from future_urban_scene_generation_amd.pipeline import broadcast_state_dicts, load_schema
        from future_urban_scene_generation_amd.synth import synth_state_dict
        nets = ("hg", "icn", "vunet") + (("edge", "inpaint") if args.inpaint else ())
        mine = {n: synth_state_dict(n, load_schema(n), 0) for n in nets} if rank == 0 else None
        t_b = time.perf_counter()
        sds = broadcast_state_dicts(mine, nets=nets, device=coll_dev)
        bcast_ms = (time.perf_counter() - t_b) * 1e3
    pipe = VehiclePipeline(dev, inpaint=args.inpaint, state_dicts=sds)
    if args.vehicles:
        # strong scaling (BASELINE configs[3]: one frame's vehicles sharded over the ranks): this rank's contiguous shard
        lo, hi = shard_range(args.vehicles, rank, world)
        args.batch, n_total, first = hi - lo, args.vehicles, lo
        full = synth_batch(args.vehicles, args.res, "cpu", inpaint=args.inpaint, seed=0)
        batch = {k: v[lo:hi].to(dev) for k, v in full.items()}
        del full
        from future_urban_scene_generation_amd import ops as _o
        for k, cp in (("hg_x", 4), ("icn_x", 24), ("vu_x", 8), ("vu_y", 4)):      # NHWC-physical, like synth_batch(nhwc=True)
            batch[k] = _o.as_nhwc(batch[k].contiguous(), cpad=cp)
    else:
        batch = synth_batch(args.batch, args.res, dev, inpaint=args.inpaint, seed=rank, nhwc=True)
        n_total, first = args.batch * world, rank * args.batch
    # VUnet noise: one stream per vehicle, seeded by the vehicle's global index, so that the images do not depend
    # on how the vehicles are spread over ranks
    seeds = [1000 + first + i for i in range(args.batch)]
    gather_ms = []
    compiled = {}

    def step():
        # check="async": the range guard's status word is read once, after the timed steps (pipe.finish()), instead of
        # synchronising the host after every pass
        if args.replay and os.environ.get("FUSG_STREAMS", "1") != "0":
            cp = compiled.get(ops.PRECISION)
            if cp is None:
                cp = compiled[ops.PRECISION] = pipe.compile(batch, seeds)
            out = cp.run(batch, vehicle_seeds=seeds, check="async")
        else:
            out = pipe.run(batch, vehicle_seeds=seeds, check="async")
        if multi:                                       # the path's only exchange: crops -> rank 0
            t_g = time.perf_counter()
            crops = torch.cat([out["icn_u8"], out["vunet_u8"]], dim=-1)
            gather_in_order(crops, n_total)
            gather_in_order(out["kp_idx"], n_total)
            gather_ms.append((time.perf_counter() - t_g) * 1e3)      # host time of the enqueue (RCCL is asynchronous)
        return out

    def barrier():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    scale = (args.res / 256.0) ** 2
    gflop_crop = (GFLOP_PER_CROP["hg"] + GFLOP_PER_CROP["icn"] + GFLOP_PER_CROP["vunet_first"] +
                  ((GFLOP_PER_CROP["edge"] + GFLOP_PER_CROP["inpaint"]) if args.inpaint else 0.0)) * scale

    def keep_settling(t_s):
        # every rank must run the same number of steps (a step contains collectives): rank 0's clock decides
        go = torch.tensor([1 if time.perf_counter() - t_s < args.settle_s else 0], dtype=torch.int32, device=coll_dev)
        if multi:
            dist.broadcast(go, src=0)
        return bool(go.item())

    def run_leg(prec, sampler=None):
        """The full protocol for one precision: settle, W warm-up steps, K timed steps, then the roofline pass."""
        ops.set_precision(prec)
        if sampler:
            sampler.start()
        # Clock settle, before (and on top of) the W warm-up steps: the card's DVFS needs ~0.5 s of load to reach its
        # steady operating point (a burst right after start-up reads 5-20 % slow or fast), and lazy
        # initialisation (plan upload, stream creation, RCCL communicators) happens in the first step.
        step()
        torch.cuda.synchronize()
        settle, t_s = 1, time.perf_counter()
        while keep_settling(t_s):
            step()
            torch.cuda.synchronize()
            settle += 1
        for _ in range(args.warmup):
            step()
        barrier()
        pipe.finish()                                   # clear the range status before the timed region
        del gather_ms[:]
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        barrier()
        dt = time.perf_counter() - t0
        out_of_range = pipe.finish()                    # one 4-byte read for all K steps
        if args.dump_outputs and rank == 0:             # host copies now: a replayed plan reuses its output tensors
            leg_outputs[prec] = {k: v.detach().cpu() for k, v in out.items()}
        # Roofline pass: the SAME K steps again with one HIP-event pair around every conv launch, recorded on
        # the launch stream.  Kept out of the timed region above because ~460 event records per step cost
        # ~10 % of wall time; kernel durations themselves are unaffected (rocprofv3 agrees, profiles/).
        # The branches of the pass are serialised for this leg (FUSG_STREAMS=0): kernels that share the GPU with
        # another stream's kernels would each read longer than they are.
        roofline = None
        if args.full and not args.no_prof:
            streams_env = os.environ.get("FUSG_STREAMS")
            os.environ["FUSG_STREAMS"] = "0"
            step()
            barrier()
            ops.prof_reset()
            ops.prof_enable(True)
            for _ in range(args.steps):
                step()
            barrier()
            ops.prof_enable(False)
            if streams_env is None:
                del os.environ["FUSG_STREAMS"]
            else:
                os.environ["FUSG_STREAMS"] = streams_env
            conv_ms, conv_launches, launched_flops = ops.prof_read(0)
            alg_flops = gflop_crop * 1e9 * args.batch * args.steps          # this rank's conv work in the timed region
            achieved = alg_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
            executed = launched_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
            traffic, tsrc = None, None
            tpath = os.path.join(REPO, "profiles", "hbm_traffic_latest.json")
            leg_key = "%s_%d%s" % (prec, args.res, "_inpaint" if args.inpaint else "")
            if os.path.exists(tpath):
                try:
                    tj = json.load(open(tpath))
                    tj = tj.get("legs", {}).get(leg_key) or (tj if leg_key == "f16x3_256" else None)
                    if tj:
                        traffic = tj.get("conv_bytes_per_launch")
                        tsrc = "NOT measured in this run (PMC counters need their own rocprofv3 pass): %s [%s], collected %s" % (
                            "profiles/hbm_traffic_latest.json", leg_key, tj.get("collected", "in an earlier run"))
                except (OSError, ValueError):
                    traffic = None
            if prec == "f32":
                kern, peak, note = "fusg::conv_igemm_f32 (all tile instantiations)", PEAK_F32_MFMA_TFLOPS, \
                    "fp32 MFMA: 1 matrix FLOP per algorithmic FLOP"
            elif prec == "bf16":
                kern, peak, note = "fusg::conv_halo_h3<..., bf16> + f16x3 kernels for the rest", PEAK_F16_MFMA_TFLOPS, \
                    ("single-pass bf16 on the halo-kernel layers: 1 matrix FLOP per algorithmic FLOP there (peak = dense bf16 MFMA "
                     "2500 TFLOP/s); the hourglass and the non-halo layers still cost 3.  Counters (profiles/r03_*bf16*): neither "
                     "pipe bounds this leg - MFMA pipe 0.19 busy on its halo launches, HBM 1.9 TB/s = 0.23 of 8 - its waves wait "
                     "(52 % of their cycles in s_waitcnt / barriers); 'bound' names only the pipe the FLOPs are priced on")
            else:
                kern, peak, note = "fusg::conv_halo_h3 + hg_bneck_h3 + conv_tapunit_h3 + conv_igemm_h3 (all instantiations)", round(PEAK_F16_MFMA_TFLOPS / 3, 1), \
                    ("split-fp16: every fp32 FLOP costs 3 fp16 matrix FLOPs (ah*wh + ah*wl + al*wh'); peak = dense "
                     "fp16 MFMA peak 2500 TFLOP/s / 3, so frac is the matrix-pipe utilisation")
            hbm_extra = {}
            if prec == "bf16" and traffic:
                # with fp32 activations the HBM bytes do not shrink with the arithmetic: report the leg against that ceiling too
                step_bytes = traffic * (conv_launches // max(1, args.steps))
                hbm_extra = {"hbm_bytes_per_step": round(step_bytes), "hbm_tb_per_s": round(step_bytes / (conv_ms / args.steps * 1e-3) / 1e12, 3),
                             "hbm_frac_of_8tb": round(step_bytes / (conv_ms / args.steps * 1e-3) / 8e12, 4)}
            roofline = {"bound": "mfma", "kernel": kern,
                        "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                        "frac": round(achieved / peak, 4),
                        "achieved_executed": round(executed, 2), "frac_executed": round(executed / peak, 4),
                        "traffic": traffic, "traffic_source": tsrc, "note": note,
                        "executed_note": "FLOPs as launched (2*M*Cout*K_pad per launch): the ICN decoder's phase form does 2.8x "
                                         "fewer MACs than the reference's 25-tap form that `achieved` prices",
                        "measured": "second pass of the same K steps, branches serialised on one stream, one HIP-event pair per launch",
                        "launches_per_step": conv_launches // max(1, args.steps),
                        "avg_launch_us": round(conv_ms * 1e3 / max(1, conv_launches), 2),
                        "conv_ms_per_step": round(conv_ms / args.steps, 3),
                        "alg_gflop_per_launch": round(gflop_crop * args.batch * args.steps / max(1, conv_launches), 3)}
            roofline.update(hbm_extra)
        power = sampler.stop() if sampler else None
        tstat = torch.tensor([dt, -dt, 1.0 if out_of_range else 0.0], dtype=torch.float64, device=coll_dev)
        if multi:
            dist.all_reduce(tstat, op=dist.ReduceOp.MAX)
        dt_max, dt_min, bad = float(tstat[0]), -float(tstat[1]), bool(tstat[2] > 0)
        leg = {"value": round(n_total * args.steps / dt_max, 3), "unit": "crops/s",
               "ms_per_step": round(dt_max / args.steps * 1e3, 3), "dtype": DTYPE[prec], "roofline": roofline,
               "settle_steps": settle, "range_status_raised": bad}
        if multi:
            leg["per_rank_crops_per_s"] = {"min": round(args.batch * args.steps / dt_max, 2),
                                           "max": round(args.batch * args.steps / dt_min, 2)}
            leg["gather_enqueue_ms_per_step"] = round(sum(gather_ms) / max(1, len(gather_ms)), 3)
        if power is not None:
            leg["power"] = power
        return leg

    precision = args.precision or ("all" if args.full else "f16x3")
    legs_wanted = {"both": ["f16x3", "f32"], "all": ["f16x3", "f32", "bf16"]}.get(precision, [precision])
    leg_outputs = {}
    sampler = None
    if args.full and rank == 0 and world == 1:
        pr = torch.cuda.get_device_properties(local_rank)
        bdf = None
        if all(hasattr(pr, a) for a in ("pci_domain_id", "pci_bus_id", "pci_device_id")):
            bdf = "%04x:%02x:%02x." % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        sampler = PowerSampler(bdf)
    legs = {}
    for i, prec in enumerate(legs_wanted):
        legs[prec] = run_leg(prec, sampler if i == 0 else None)
    head = legs_wanted[0]
    if legs[head]["range_status_raised"]:
        # cannot happen with the synthetic inputs; if it does, the f16x3 figure is not a valid measurement
        if head != "f32" and "f32" not in legs and args.precision is None:
            legs["f32"] = run_leg("f32")            # a plain run: the f32 leg that --full would have timed anyway
        if "f32" in legs and head != "f32":
            head = "f32"
        else:
            raise SystemExit("bench.py: the f16x3 range status was raised during the timed steps - leg invalid")
    ops.set_precision(head)
    if args.dump_outputs and rank == 0:
        shapes = dump_outputs(leg_outputs[head], args.dump_outputs)
        print("bench.py: outputs of the last timed %s step -> %s: %s" % (head, args.dump_outputs, json.dumps(shapes)),
              file=sys.stderr, flush=True)
    leg_outputs.clear()

    extra = {}
    if args.full and rank == 0 and world == 1 and not args.no_clip and not args.inpaint:
        # secondary figure: clip mode = 1 HG + 6 ICN + 1 VUnet-full + 5 VUnet-later per vehicle,
        # 8 vehicles x 6 frames per pass (ICN and the VUnet shape half run at batch 48)
        from future_urban_scene_generation_amd.pipeline import synth_clip
        V, F = 8, 6
        clip = synth_clip(V, F, args.res, dev)
        pipe.run_clip(clip, check="async")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            pipe.run_clip(clip, check="async")
        bad = pipe.finish()
        cdt = (time.perf_counter() - t1) / 3
        extra["clip_mode"] = {"vehicles": V, "frames": F, "ms_per_pass": round(cdt * 1e3, 3),
                              "vehicle_clips_per_s": round(V / cdt, 2), "frames_per_s": round(V * F / cdt, 1),
                              "range_status_raised": bool(bad)}
        del clip
    if args.full and rank == 0 and world == 1 and not args.no_clip and args.res == 256:
        # secondary figure: frame mode = the chained per-frame driver (VehiclePipeline.run_frame: detector boxes -> box
        # crops -> hourglass -> argmax -> pose fit, plane warps -> ICN inputs -> ICN -> Lab image, VUnet inputs -> VUnet,
        # resize-back + ordered paste of every vehicle), 8 vehicles on a 720 x 1280 frame, everything device-resident;
        # the host part per frame = the 2 x 5 homography fits per vehicle and the pose fit's 4 x 7-number epilogue
        from future_urban_scene_generation_amd.pipeline import synth_frame
        FV = 8
        scene = synth_frame(FV, (720, 1280), dev, seed=3, inpaint=bool(args.inpaint))
        scene["vehicle_seeds"] = list(range(FV))
        fms = {}
        for mode, rep in (("eager", False), ("replay", True)):
            pipe.run_frame(scene, replay=rep)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(5):
                pipe.run_frame(scene, replay=rep)
            torch.cuda.synchronize()
            fms[mode] = (time.perf_counter() - t1) / 5
        # a sequence of frames (two scenes alternating), one frame in flight while the next is issued: run_frames
        scene2 = synth_frame(FV, (720, 1280), dev, seed=4, inpaint=bool(args.inpaint))
        scene2["vehicle_seeds"] = list(range(100, 100 + FV))
        for _ in pipe.run_frames([scene, scene2, scene]):
            pass
        torch.cuda.synchronize()
        NF = 12
        t1 = time.perf_counter()
        for _ in pipe.run_frames([scene, scene2] * (NF // 2)):
            pass
        torch.cuda.synchronize()
        fdt = (time.perf_counter() - t1) / NF
        extra["frame_mode"] = {"vehicles": FV, "frame": "720x1280", "ms_per_frame": round(fdt * 1e3, 3),
                               "vehicles_per_s": round(FV / fdt, 2),
                               "ms_per_frame_one_at_a_time": round(fms["replay"] * 1e3, 3),
                               "ms_per_frame_one_at_a_time_eager": round(fms["eager"] * 1e3, 3),
                               "issue": "run_frames over 12 frames: networks as one recorded-plan replay, frame i+1 issued "
                                        "before frame i's pose / range status are read back (pinned, one event per frame); "
                                        "run_frame (one synchronous frame at a time) beside it",
                               "includes": "box crops, hourglass + argmax + pose fit, plane warps, ICN (+Lab->BGR), VUnet, "
                                           + ("EdgeConnect on every vehicle's box + its resize-back under the pasted crop, " if args.inpaint else "")
                                           + "paste-back of both composited frames; range check per frame"}
        # clip mode of the frame driver: one vehicle clip the reference's way - the first frame through
        # run_frame, its five future frames (trajectory_inference.py:267) through run_later_frame with the first frame's state
        from future_urban_scene_generation_amd.pipeline import synth_later_frame
        laters = [synth_later_frame(scene, 1 + n) for n in range(5)]
        for _ in pipe.run_clip_frames(scene, laters, replay=True):
            pass
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        NC = 3
        for _ in range(NC):
            for _ in pipe.run_clip_frames(scene, laters, replay=True):
                pass
        torch.cuda.synchronize()
        cdt = (time.perf_counter() - t1) / NC
        extra["clip_frame_mode"] = {"vehicles": FV, "frames": 6, "ms_per_clip": round(cdt * 1e3, 3), "ms_per_frame": round(cdt * 1e3 / 6, 3),
                                    "vehicle_frames_per_s": round(FV * 6 / cdt, 1),
                                    "what": "run_clip_frames: 1 run_frame (synchronous) + 5 later frames through run_later_frames (no hourglass / "
                                            "pose fit / appearance encoder; one later frame in flight: frame i+1's homography fits and launches "
                                            "are issued before frame i's range status is read back), 8 vehicles on a 720 x 1280 frame"}
        del scene, scene2
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_baseline, quality = cpu_baseline_leg(args, batch, pipe, torch)
        extra.update(quality)
    if args.full and rank == 0 and world == 1 and not args.no_clip and not args.inpaint and args.res == 256:
        extra["configs0_vunet_forward_b1"] = vunet_forward_leg(args, pipe, torch, with_cpu=not args.no_cpu_baseline,
                                                               threads=cpu_baseline["cores"] if cpu_baseline else None)

    if rank == 0:
        h = legs[head]
        line = {"metric": "synthesised vehicle crops/sec @%dx%d" % (args.res, args.res), "value": h["value"], "unit": "crops/s",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": h["ms_per_step"], "higher_is_better": True, "scaling": "strong" if args.vehicles else "weak",
                "vs_baseline": None, "dtype": h["dtype"], "data": "synthetic",
                "config": {"workload": ("configs[2]: batch=%d %dx%d crops/GPU, hourglass->warp_learn(ICN)->vunet + edgeconnect"
                                        if args.inpaint else
                                        "configs[1]: batch=%d %dx%d crops/GPU, hourglass->warp_learn(ICN)->vunet first-frame") % (args.batch, args.res, args.res)
                                       + (" | strong scaling: %d vehicles of one frame sharded over the ranks (configs[3])" % args.vehicles if args.vehicles else ""),
                           "batch_per_gpu": args.batch, "res": args.res, "inpaint": bool(args.inpaint), "precision": head,
                           "gflop_per_crop": round(gflop_crop, 2), "sharding": "vehicles over ranks, gather of uint8 crops to rank 0",
                           "inputs": "device-resident fp32, NHWC-physical with zero-padded channel pitch (what the frame driver's glue "
                                     "kernels write; a caller with standard NCHW tensors pays four conversion launches per pass)"},
                "roofline": h["roofline"], "cpu_baseline": cpu_baseline,
                "precision_legs": {k: {kk: vv for kk, vv in v.items() if kk != "power"} for k, v in legs.items()}}
        if multi:
            # "rccl_ranks" only when RCCL ("nccl" on ROCm) really carried the collectives; a gloo rehearsal says "dist_ranks"
            line["rccl_ranks" if dist.get_backend() == "nccl" else "dist_ranks"] = dist.get_world_size()
            line["dist_backend"] = dist.get_backend()
            line["per_rank_crops_per_s"] = h.get("per_rank_crops_per_s")
            line["gather_enqueue_ms_per_step"] = h.get("gather_enqueue_ms_per_step")
            line["weights"] = ("broadcast from rank 0 (%.0f ms, one flat blob per network)" % bcast_ms) if bcast_ms is not None \
                else "every rank builds them from the seed (--no-broadcast-weights)"
            line["host_threads_per_rank"] = torch.get_num_threads()
        line.update(extra)
        if h.get("power") is not None:
            line["power"] = h["power"]
        line["settle_steps"] = h["settle_steps"]
        line["streams"] = "serial" if os.environ.get("FUSG_STREAMS", "1") == "0" else "one HIP stream per network branch (+ one for the VUnet's shape encoder)"
        line["issue"] = "recorded plan replay (fusg_plan_run)" if args.replay else "eager (one ctypes call per launch)"
        print(json.dumps(line), flush=True)
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Benchmark of the MDCT + psychoacoustic-masking hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

With N > 1 and no torchrun environment this process starts N ranks itself (``python -m torch.distributed.run``, one
process per GPU) *before it makes any GPU call*, relays rank 0's JSON line and exits with the children's status; under
torchrun (RANK / WORLD_SIZE set) it is one of those ranks.  A mismatch between --gpus and the world size is an error.

One "step" = one pass of the hot path over one batch of synthetic PCM resident in HBM:
fused encode (x -> X, tonality, threshold; one HIP kernel) followed by decode (X -> x^; one HIP kernel).
Workload: N = 1 is BASELINE.json configs[1] at its roofline length: 256 stereo 48 kHz clips of
K = 468 blocks (10 s), filters_n = 1024 -- 3.9 GB touched per step, far beyond the 256 MiB Infinity Cache.  N > 1 is
configs[2]: every rank holds its 512-clip share of B = 4096 / 8 (weak scaling: the share per GPU is the same at
N = 2, 4, 8).  Clips are independent (reference mdctransformer.py:292-295 folds channels into the batch axis), so the
batch axis is sharded and there is no data-path collective; RCCL carries the barrier, the max-over-ranks time and the
reduction of frame counts / checksums / round-trip error.

The timed step is the call shape of the reference's classes: X, t, thr = codec.encode(x); x^ = codec.decode(X) -- the
library allocates (and places, audiocodec_amd/placement.py) what it returns, as mdctransformer.py:62-125 and
psychoacoustic.py:102-148 return new tensors.  The same step on caller-owned plain torch tensors (encode_into /
decode_into: what a C-ABI caller that brings its own buffers gets) is reported beside it (caller_owned_*).  Prints ONE
JSON line on rank 0.  value = frames/s over all GPUs, a frame being one 1024-sample hop of one channel, encode + decode
both done (20 484 algorithmic bytes per frame).
"""

import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 1024
ENC_BYTES = 4 * N + (4 * N + 4 * N + 4)      # PCM in; X, thr, tonality out           = 12 292 B / frame
DEC_BYTES = 4 * N + 4 * N                    # X in; PCM out                          =  8 192 B / frame
HBM_PEAK_GBS = 8000.0                        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
CLIPS_1GPU = 256                             # BASELINE configs[1]
CLIPS_PER_RANK = 4096 // 8                   # BASELINE configs[2]: B = 4096 over 8 GPUs


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)    # warm-up 10 iterations, then >= 200 timed
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--clips", type=int, default=0,
                    help="stereo clips per GPU; 0 = 256 at --gpus 1 (configs[1]), 512 = 4096 / 8 otherwise (configs[2])")
    ap.add_argument("--blocks", type=int, default=468, help="blocks (hops) per clip; 468 = 10 s at 48 kHz")
    ap.add_argument("--no-workspace", action="store_true",
                    help="skip the side measurement of the same step on audiocodec_amd.Workspace-placed tensors")
    ap.add_argument("--settle-ms", type=float, default=100.0,
                    help="keep the device busy with the same step for this long before the warmup steps: an MI355X that "
                         "has idled runs the first ~30 ms of load at reduced clocks (reported as settle_ms / settle_steps; "
                         "cold_start in the same line is the same measurement without it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-encode-api", action="store_true", help="(accepted for old command lines: the allocating API is the headline now)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the side measurements (f32 spreading, "
                    "K = 46, configs[3] / configs[4])")
    ap.add_argument("--no-smi", action="store_true", help="do not sample the GPU's clocks / power from a side process")
    ap.add_argument("--dist", choices=("auto", "nccl", "gloo", "none"), default="auto",
                    help="process group of the ranks: auto = RCCL (\"nccl\") under torch.distributed.run -- also for ONE rank, "
                         "so that `torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` sends the barrier and the scalar "
                         "reductions through RCCL on the device -- and none for a plain `python bench.py`; nccl / gloo: start "
                         "the ranks (even one) under torch.distributed.run with that backend; AC_BENCH_FORCE_DIST=1 = --dist nccl")
    ap.add_argument("--dry-run-launch", action="store_true",
                    help="print the torch.distributed.run command and backend this call would start its ranks with, as JSON, "
                         "and exit (no GPU call)")
    ap.add_argument("--side-json", default="", help="also write the side measurements (the earlier stdout line) to this file")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the headline step returned in its last step (X, tonality and "
                         "threshold of encode(), the PCM of decode(); rank 0's clips) as DIR/<name>.npy, float32: in full "
                         "when small, else a fixed seeded sample of the flattened output (dump_indices()), < 64 MB in all")
    return ap.parse_args(argv)


# ---- N > 1 without torchrun: start the ranks from here, before anything touches the GPU ---------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def plan_launch(gpus, have, dist, env, argv, port):
    """The command and environment `python bench.py --gpus N` starts its N ranks with (pure: no GPU call, testable on
    CPU).  RCCL ("nccl") when the box has a device per rank; with fewer devices the ranks share them over gloo (rehearsal
    only) unless a backend was asked for explicitly (--dist / AC_BENCH_BACKEND), in which case the ranks themselves refuse
    an impossible combination (a rank without its own device under nccl exits non-zero)."""
    env_add = {}
    backend = env.get("AC_BENCH_BACKEND") or (dist if dist in ("nccl", "gloo") else None)
    if backend is None:
        backend = "nccl" if have >= gpus else "gloo"
    env_add["AC_BENCH_BACKEND"] = backend
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return {"cmd": cmd, "env": env_add, "backend": backend, "devices": have, "ranks": gpus}


def launch_ranks(args):
    """Re-run this script as `--gpus N` ranks under torch.distributed.run (children of this GPU-free process) and
    relay their output.  Never an exec: the ranks are child processes, this process exits with their status."""
    import torch
    have = torch.cuda.device_count()          # (counting devices does not initialise the GPU on this image)
    argv = [a for a in sys.argv[1:] if a != "--dry-run-launch"]
    for i, a in enumerate(argv):   # the ranks run from ROOT: they get --dump-outputs as this process resolved it
        if a.startswith("--du"):   # (argparse takes any unambiguous prefix of --dump-outputs)
            if "=" in a:
                argv[i] = "--dump-outputs=" + args.dump_outputs
            elif i + 1 < len(argv):
                argv[i + 1] = args.dump_outputs
    plan = plan_launch(args.gpus, have, args.dist, os.environ, argv, free_port())
    if args.dry_run_launch:
        print(json.dumps(plan))
        return 0
    if have <= 0:
        sys.exit("bench.py needs the MI355X (no HIP device visible)")
    return subprocess.run(plan["cmd"], env=dict(os.environ, **plan["env"]), cwd=ROOT).returncode


# ---- CPU baseline (oracle, host cores) -------------------------------------------------------------------------------
def cpu_share():
    """How many single-threaded oracle processes the CPU baseline may start, and which bound set it: the scheduler affinity
    of this process, a cgroup cpu.max / cfs quota when one is set, and the pool's rule for a GPU box -- worker pools are
    sized to the box's CPU share, 16 per GPU (a 1-GPU box shares a 256-core host with seven other tenants; no cgroup quota
    enforces that, so it is applied here).  AC_BENCH_CPU_PROCS overrides."""
    host = os.cpu_count() or 1
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = host
    quota = None
    try:   # cgroup v2, then v1
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = float(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = float(f.read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    try:
        import torch
        gpus = max(1, torch.cuda.device_count())   # (counting devices does not initialise the GPU on this image)
    except Exception:
        gpus = 1
    bounds = {"affinity": affinity, "pool_share_16_per_gpu": 16 * gpus}
    if quota is not None:
        bounds["cgroup_cpu_quota"] = max(1, int(quota))
    forced = os.environ.get("AC_BENCH_CPU_PROCS")
    if forced:
        bounds = {"AC_BENCH_CPU_PROCS": max(1, int(forced))}
    name = min(bounds, key=lambda k: bounds[k])
    return {"processes": max(1, bounds[name]), "bound": name, "host_cpus": host, "affinity_cpus": affinity,
            "cgroup_cpu_quota": quota, "visible_gpus": gpus}


def cpu_baseline(seconds=12.0):
    """The oracle (closed-form numpy/scipy restatement, oracle/audiocodec_oracle.py) timed on the host cores on a
    bounded sample of the same workload: single-threaded processes (oracle/cpu_bench.py), each looping encode + decode
    over stereo clips of 46 blocks for `seconds`; frames/s summed over the processes.  Runs before this process touches
    the GPU (child processes are started from a GPU-free parent)."""
    share = cpu_share()
    host_cpus, usable, procs_n = share["host_cpus"], share["affinity_cpus"], share["processes"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
               OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "oracle.cpu_bench", "--seconds", str(seconds)]
    procs = [subprocess.Popen(cmd + ["--seed", str(i)], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
             for i in range(procs_n)]
    rate, frames = 0.0, 0
    for p in procs:
        out, _ = p.communicate(timeout=seconds * 6 + 120)
        r = json.loads(out.strip().splitlines()[-1])
        rate += r["frames"] / r["seconds"]
        frames += r["frames"]
    # the reference-shaped flavour (dense [2,N,N] polyphase products, 2N-point DCT-III, dense Bark einsums, materialised
    # 5-D masking tensor: the op sequence the reference hands to TensorFlow) on the same cores
    dense_s = 8.0
    dprocs = [subprocess.Popen(cmd[:-1] + [str(dense_s), "--dense", "--seed", str(i)], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True)
              for i in range(procs_n)]
    drate, dframes, dsec = 0.0, 0, 0.0
    for p in dprocs:
        out, _ = p.communicate(timeout=dense_s * 10 + 300)
        r = json.loads(out.strip().splitlines()[-1])
        drate += r["frames"] / r["seconds"]
        dframes += r["frames"]
        dsec = max(dsec, r["seconds"])
    return {
        "value": rate, "unit": "frames/s", "cores": procs_n, "kind": "port",
        "host_cpus": host_cpus, "usable_cpus": usable, "processes": procs_n, "threads_per_process": 1,
        "cores_bound": share["bound"], "cgroup_cpu_quota": share["cgroup_cpu_quota"], "visible_gpus": share["visible_gpus"],
        "sample": "%d single-threaded processes x %.0f s of (B=2 stereo clips, K=46 blocks, N=%d) encode+decode, "
                  "closed-form numpy/scipy oracle; %d frames in total" % (procs_n, seconds, N, frames),
        "reference_shaped_value": drate, "reference_shaped_cores": procs_n,
        "reference_shaped_value_per_core": drate / procs_n,
        "reference_shaped_sample": "%d single-threaded processes x %.1f s, dense polyphase / DCT-III / einsum restatement of the "
                                   "reference's op sequence on the same clips; %d frames in total" % (procs_n, dsec, dframes),
    }


# ---- GPU clocks / power from a side process (sysfs; started before this process touches the GPU) -------------------
_SMI_CHILD = r"""
import glob, json, os, sys, time
def rd(p):
    try:
        with open(p) as f: return f.read().strip()
    except Exception: return None
def cur(p):   # pp_dpm_*: the line marked '*'
    s = rd(p)
    if not s: return None
    for line in s.splitlines():
        if line.rstrip().endswith('*'):
            try: return float(line.split(':')[1].strip().rstrip('*').strip().lower().replace('mhz', ''))
            except Exception: return None
    return None
cards = []   # every card with a hwmon directory (one per physical GPU), keyed by its PCI address
for d in sorted(glob.glob('/sys/class/drm/card*/device')):
    hw = sorted(glob.glob(d + '/hwmon/hwmon*'))
    if hw: cards.append((os.path.basename(os.path.realpath(d)), d, hw[0]))
only = sys.argv[3] if len(sys.argv) > 3 else ''
out = open(sys.argv[1], 'w')
stop = sys.argv[2]
t_end = time.time() + 900
while time.time() < t_end and not os.path.exists(stop):
    for bdf, dev, hw in cards:
        if only and only.lower() not in bdf.lower(): continue
        s = {'t': time.time(), 'bdf': bdf, 'sclk_mhz': cur(dev + '/pp_dpm_sclk'), 'mclk_mhz': cur(dev + '/pp_dpm_mclk'),
             'fclk_mhz': cur(dev + '/pp_dpm_fclk'), 'busy': rd(dev + '/gpu_busy_percent')}
        for k, f in (('power_uw', 'power1_input'), ('freq_hz', 'freq1_input'), ('temp_mc', 'temp2_input')):
            v = rd(hw + '/' + f)
            if v is not None: s[k] = v
        out.write(json.dumps(s) + '\n')
    out.flush()
    time.sleep(0.002)
"""


class SmiSampler:
    """Polls the amdgpu sysfs files (current sclk / mclk level, hwmon power) every ~2 ms from a child process."""

    def __init__(self):
        import tempfile
        self.dir = tempfile.mkdtemp(prefix="ac_smi_")
        self.log, self.stop = os.path.join(self.dir, "log.jsonl"), os.path.join(self.dir, "stop")
        self.p = subprocess.Popen([sys.executable, "-c", _SMI_CHILD, self.log, self.stop],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def finish(self, t0, t1, bdf=None):
        """Stops the child; summary of the samples of the GPU at PCI address `bdf` taken inside the wall-clock window
        [t0, t1] (and in the half second before it)."""
        open(self.stop, "w").close()
        try:
            self.p.wait(timeout=5)
        except Exception:
            self.p.kill()
        rows = []
        try:
            with open(self.log) as f:
                rows = [json.loads(line) for line in f if line.strip()]
        except Exception:
            pass
        seen = sorted({r.get("bdf") for r in rows})
        if bdf is not None:
            rows = [r for r in rows if bdf.lower() in str(r.get("bdf", "")).lower()]
        inside = [r for r in rows if t0 <= r["t"] <= t1]
        before = [r for r in rows if t0 - 0.5 <= r["t"] < t0]

        def stat(sel, key, scale=1.0):
            v = []
            for r in sel:
                try:
                    v.append(float(r[key]) * scale)
                except Exception:
                    pass
            return {"n": len(v), "min": min(v), "mean": sum(v) / len(v), "max": max(v)} if v else None

        out = {"source": "amdgpu sysfs (pp_dpm_*, hwmon) polled from a side process", "pci": bdf, "cards_seen": len(seen),
               "samples_in_timed_region": len(inside)}
        for name, sel in (("timed_region", inside), ("half_second_before", before)):
            out[name] = {"sclk_mhz": stat(sel, "sclk_mhz"), "mclk_mhz": stat(sel, "mclk_mhz"),
                         "fclk_mhz": stat(sel, "fclk_mhz"), "power_w": stat(sel, "power_uw", 1e-6),
                         "freq1_mhz": stat(sel, "freq_hz", 1e-6), "gpu_busy_percent": stat(sel, "busy")}
        if not rows or all(v is None for v in out["timed_region"].values()):
            out["note"] = "no readable amdgpu sysfs counters on this box" if not rows or "sclk_mhz" not in rows[0] \
                else "no sample fell inside the timed region"
        return out


def measured_traffic():
    """HBM bytes per launch of the fused encode kernel from the committed PMC passes (profiles/<round>/traffic.json:
    FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md + WRITE_SIZE) and the file it came from, or None.
    NOT a counter of this run: the contract line labels it (roofline.traffic_source)."""
    best = None
    prof = os.path.join(ROOT, "profiles")
    if os.path.isdir(prof):
        for r in sorted(os.listdir(prof)):
            f = os.path.join(prof, r, "traffic.json")
            if os.path.exists(f):
                with open(f) as fh:
                    best = (json.load(fh), "profiles/%s/traffic.json" % r)
    return best


def make_clips(torch, dev, first_clip, clips, blocks, channels=2, n=N):
    """Synthetic PCM, uniform(-1, 1), one Philox stream per GLOBAL clip index (seed 1234 + index): rank r of a sharded
    run generates exactly the clips [first_clip, first_clip + clips) a single rank would hold at those positions, so
    checksums reduced over the ranks can be compared with a one-rank run over the same clips."""
    x = torch.empty((clips, blocks * n, channels), device=dev, dtype=torch.float32)
    gen = torch.Generator(device=dev)
    for b in range(clips):
        gen.manual_seed(1234 + first_clip + b)
        x[b].uniform_(-1.0, 1.0, generator=gen)
    return x


def run_steps(torch, codec, x, X, t, thr, xh, n, timed=False):
    """Enqueues n steps (encode launch + decode launch); with timed=True returns per-step kernel times by events on the
    stream the kernels run on (after a synchronisation)."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)] if timed else None
    for i in range(n):
        if timed:
            ev[i][0].record()
        codec.encode_into(x, X, t, thr)
        if timed:
            ev[i][1].record()
        codec.decode_into(X, xh)
        if timed:
            ev[i][2].record()
    if not timed:
        return None
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]) for e in ev], [e[1].elapsed_time(e[2]) for e in ev]


def settle(torch, codec, x, X, t, thr, xh, settle_ms):
    """Keeps the device busy with the step for `settle_ms` (no idle gap longer than a synchronisation).  An MI355X that
    has idled for more than ~5 ms runs the first ~30 ms of any sustained load at reduced clocks (DESIGN_LOG.md section 5a,
    tools/ramp_probe2.py / ramp_probe3.py: steps 3..30 after an idle gap take up to 25 % longer, whatever ran before the
    gap); a warm-up of 5 steps ends in the middle of that.  Returns the number of steps run."""
    if settle_ms <= 0:
        return 0
    n, t0 = 0, time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < settle_ms:
        run_steps(torch, codec, x, X, t, thr, xh, 8)
        torch.cuda.synchronize()
        n += 8
    return n


def timed_loop(torch, codec, x, X, t, thr, xh, steps, warmup, barrier=None, settle_ms=0.0):
    """Device settle (see settle()), `warmup` untimed steps, then exactly `steps` steps between synchronisations; per-step
    kernel times by events.  Returns (elapsed_s, encode_ms list, decode_ms list, t0, t1 wall clock, settle steps)."""
    settled = settle(torch, codec, x, X, t, thr, xh, settle_ms)
    run_steps(torch, codec, x, X, t, thr, xh, warmup)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    if barrier is not None:
        barrier()
    torch.cuda.synchronize()
    w0 = time.time()
    t0 = time.perf_counter()
    for i in range(steps):
        ev[i][0].record()
        codec.encode_into(x, X, t, thr)
        ev[i][1].record()
        codec.decode_into(X, xh)
        ev[i][2].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    w1 = time.time()
    enc = [e[0].elapsed_time(e[1]) for e in ev]
    dec = [e[1].elapsed_time(e[2]) for e in ev]
    return elapsed, enc, dec, w0, w1, settled


def timed_loop_api(torch, codec, x, steps, warmup, barrier=None, settle_ms=0.0):
    """The step as a user of the reference's classes calls it -- X, t, thr = codec.encode(x); x^ = codec.decode(X): the library
    allocates (and places, audiocodec_amd/placement.py) what it returns (mdctransformer.py:62-125, psychoacoustic.py:102-148
    return new tensors).  Device settle, `warmup` untimed steps, then exactly `steps` steps between synchronisations; per-launch
    times by events.  Returns (elapsed_s, encode_ms list, decode_ms list, t0, t1 wall clock, settle steps, last outputs)."""
    def step(ev=None):
        if ev:
            ev[0].record()
        X, t, thr = codec.encode(x)
        if ev:
            ev[1].record()
        xh = codec.decode(X)
        if ev:
            ev[2].record()
        return X, t, thr, xh
    t0 = time.perf_counter()
    n_settle = 0
    while (time.perf_counter() - t0) * 1e3 < settle_ms:
        for _ in range(8):
            step()
        torch.cuda.synchronize()
        n_settle += 8
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    if barrier is not None:
        barrier()
    torch.cuda.synchronize()
    w0 = time.time()
    t0 = time.perf_counter()
    out = None
    for i in range(steps):
        out = step(evs[i])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    w1 = time.time()
    enc = [e[0].elapsed_time(e[1]) for e in evs]
    dec = [e[1].elapsed_time(e[2]) for e in evs]
    return el, enc, dec, w0, w1, n_settle, out


# ---- --dump-outputs: the results of the timed path, for comparing two builds output for output ------------------------
DUMP_BUDGET_BYTES = 48 << 20     # all files together (< 64 MB), split evenly over the outputs
DUMP_SEED = 1234


def dump_indices(np, numel, keep, seed=DUMP_SEED):
    """Flat indices of the fixed sample of an output of `numel` elements: None (all of it) when numel <= keep, else one
    element drawn uniformly from each of `keep` equal strata of the flat range -- sorted, distinct, every region of the
    tensor covered.  Depends on (numel, keep, seed) only: every run and every build samples the same elements."""
    if numel <= keep:
        return None
    edges = np.arange(keep + 1, dtype=np.int64) * numel // keep
    return edges[:-1] + np.random.default_rng(seed).integers(0, edges[1:] - edges[:-1])


def dump_outputs(np, torch, outdir, arrays):
    """Writes each output (name -> device tensor) as outdir/<name>.npy in float32 (float64 stays float64), in full or as
    the dump_indices() sample of the flattened tensor; returns what was written."""
    os.makedirs(outdir, exist_ok=True)
    files = {}
    for name, a in arrays.items():
        dt = torch.float64 if a.dtype == torch.float64 else torch.float32
        keep = DUMP_BUDGET_BYTES // (len(arrays) * (8 if dt == torch.float64 else 4))
        flat = a.detach().reshape(-1)
        idx = dump_indices(np, flat.numel(), keep)
        if idx is not None:
            flat = flat.index_select(0, torch.from_numpy(idx).to(flat.device))
        host = flat.to(dt).cpu().numpy()
        np.save(os.path.join(outdir, name + ".npy"), host if idx is not None else host.reshape(tuple(a.shape)))
        files[name] = {"shape": list(a.shape), "written": int(host.size), "sampled": idx is not None}
    return {"dir": outdir, "sample_seed": DUMP_SEED, "files": files}


def other_configs(torch, np, audiocodec_amd, dev, steps, warmup, settle_ms):
    """Side measurements beside the headline (rank 0, N = 1 only, outside the timed region): the all-float32 spreading
    product on the headline workload, the cache-resident K = 46 length of SURVEY 8(d), BASELINE configs[3] and
    configs[4] (parity-test cases first -- tests/test_gpu_parity.py -- these are their measured rates)."""
    out = {}

    def med(fn, reps=7):
        fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def alloc(B, K, n, C=2):
        return (torch.empty((B, K + 1, n, C), device=dev), torch.empty((B, K + 1, 1, C), device=dev),
                torch.empty((B, K + 1, n, C), device=dev), torch.empty((B, (K + 2) * n, C), device=dev))

    # (a) the headline step with the band x band spreading product in float32 on the vector ALU (AC_SPREAD_F32): the
    #     all-float32 number beside the default split-bf16 matrix-core form
    B, K = CLIPS_1GPU, 468
    x = make_clips(torch, dev, 0, B, K)
    X, t, thr, xh = alloc(B, K, N)
    codec32 = audiocodec_amd.AudioCodec(48000, N, spreading="f32")
    el, enc, dec, _, _, _ = timed_loop(torch, codec32, x, X, t, thr, xh, steps, warmup, settle_ms=settle_ms)
    out["f32_spreading"] = {"value": B * 2 * K * steps / el, "ms_per_step": el / steps * 1e3,
                            "encode_ms": float(np.mean(enc)), "decode_ms": float(np.mean(dec)),
                            "kernel": "k_fwd_fast<8, 0, true, 4, 0, 0>"}
    del x, X, t, thr, xh
    # (b) K = 46 (1-s clips): 96.5 MB in, 98.6 MB each for X and thr -- fits the 256 MiB Infinity Cache; reported, not
    #     used for the roofline claim
    K = 46
    codec = audiocodec_amd.AudioCodec(48000, N)
    x = make_clips(torch, dev, 0, B, K)
    X, t, thr, xh = alloc(B, K, N)
    el, enc, dec, _, _, _ = timed_loop(torch, codec, x, X, t, thr, xh, steps, warmup, settle_ms=settle_ms)
    out["k46_cache_resident"] = {"workload": "batch=256 stereo clips of K=46 blocks (1 s), N=1024", "value": B * 2 * K * steps / el,
                                 "ms_per_step": el / steps * 1e3, "encode_ms": float(np.mean(enc)),
                                 "decode_ms": float(np.mean(dec))}
    # the same steps captured once into a HIP graph and replayed: at this size the gaps between the launches are a
    # measurable share of the step (the entry points only enqueue kernels, so a caller may capture them)
    try:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            run_steps(torch, codec, x, X, t, thr, xh, 2)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run_steps(torch, codec, x, X, t, thr, xh, steps)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        elg = time.perf_counter() - t0
        out["k46_cache_resident"]["graph_replay"] = {"value": B * 2 * K * steps / elg, "ms_per_step": elg / steps * 1e3}
        del g
    except Exception as e:   # reported, not fatal: a side figure
        out["k46_cache_resident"]["graph_replay"] = {"error": "%s: %s" % (type(e).__name__, e)}
    del x, X, t, thr, xh
    # (c) configs[3]: N = 2048 long-window MDCT + masking, Bark spreading as a band x band bf16 MFMA contraction
    n, K = 2048, 234
    x = make_clips(torch, dev, 0, B, K, n=n)
    X, t, thr, xh = alloc(B, K, n)
    ref = torch.empty_like(X)
    rows, codecs = {}, {}
    for mode in ("f32", "bf16x2_mfma", "bf16_mfma"):
        codecs[mode] = audiocodec_amd.AudioCodec(48000, n, spreading=mode)
        codecs[mode].encode_into(x, X, t, thr)
        if mode == "f32":
            ref.copy_(thr)
        rows[mode] = {"thr_max_rel_dev_vs_f32": float(((thr - ref).abs() / ref).max()), "encode_ms_rounds": []}
    for _ in range(3):   # interleaved rounds, median per form
        for mode, c in codecs.items():
            rows[mode]["encode_ms_rounds"].append(med(lambda: c.encode_into(x, X, t, thr), reps=5))
    for mode in rows:
        rows[mode]["encode_ms"] = float(np.median(rows[mode].pop("encode_ms_rounds")))
    c = codecs["bf16x2_mfma"]
    dec = med(lambda: c.decode_into(X, xh))
    fr = B * 2 * K
    out["configs[3]"] = {"workload": "batch=256 stereo 48 kHz clips, N=2048, K=234 blocks (10 s)", "spreading": rows,
                         "decode_ms": dec, "bytes_per_frame_encode": 12 * n + 4, "bytes_per_frame_decode": 8 * n,
                         "frames_per_s_bf16x2_mfma": fr / ((rows["bf16x2_mfma"]["encode_ms"] + dec) * 1e-3),
                         "encode_GBs_bf16x2_mfma": (12 * n + 4) * fr / (rows["bf16x2_mfma"]["encode_ms"] * 1e-3) / 1e9}
    del x, X, t, thr, ref, xh
    # (c2) filters_n beside the powers of two (the reference takes any even filters_n, mdctransformer.py:26): the LDS-FFT tier
    #     on B = 64 stereo 10-s clips, MDCT analysis / synthesis into preallocated tensors, algorithmic 8 N bytes per frame
    rows = {}
    for n in (960, 480, 4096):
        K = 468 * 1024 // n
        m = audiocodec_amd.MDCTransformer(n)
        x = make_clips(torch, dev, 0, 64, K, n=n)
        X = m.transform(x)
        xh = m.inverse_transform(X)
        lib, plan, st = m._lib, m._plan(dev), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        px, pX, pxh = (ctypes.c_void_p(v.data_ptr()) for v in (x, X, xh))   # (the C ABI directly: no allocation in the timed calls)
        fwd = med(lambda: lib.ac_mdct_forward(plan, px, pX, 64, K, 2, st))
        inv = med(lambda: lib.ac_mdct_inverse(plan, pX, pxh, 64, K + 1, 2, st))
        fr = 64 * 2 * K
        rows[str(n)] = {"analysis_ms": fwd, "synthesis_ms": inv, "analysis_GBs": 8 * n * fr / fwd / 1e6,
                        "synthesis_GBs": 8 * n * fr / inv / 1e6}
        del x, X, xh
    out["lds_fft_tier"] = {"workload": "batch=64 stereo 48 kHz clips of 10 s, MDCT analysis / synthesis alone", "filters_n": rows}
    # (d) configs[4]: streaming overlap-add through the device-resident state, chunks of 256 blocks.  One clip gives a
    #     launch only 256 wave tasks, so a chunk costs launch + one frame's latency, not bandwidth: reported are the
    #     10-minute pass as one dependent chain (analysis, then synthesis of the same chunk, one stream), the same pipelined
    #     on two streams (analysis of chunk i+1 beside synthesis of chunk i, as a codec runs them), the host-synchronised
    #     latency of one chunk, and 64 concurrent streams (B = 64) through the same entry points.
    codec = audiocodec_amd.AudioCodec(48000, N)
    k = 256

    def stream_case(Bs, Kt, fused):
        xs = torch.rand((Bs, Kt * N, 2), device=dev) * 2 - 1
        st = codec.stream(Bs, 2)
        bufs = [(torch.empty((Bs, k, N, 2), device=dev), torch.empty((Bs, k, 1, 2), device=dev),
                 torch.empty((Bs, k, N, 2), device=dev)) for _ in range(2)]
        xo = [torch.empty((Bs, k * N, 2), device=dev) for _ in range(2)]
        chunks = [xs[:, p * N:(p + k) * N] for p in range(0, Kt - k + 1, k)]
        if Bs > 1:   # a batch of streams hands over one contiguous buffer per chunk (a slice of [B, K N, C] is not one)
            chunks = [c.contiguous() for c in chunks]
        s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        done_a = [torch.cuda.Event() for _ in range(2)]
        done_s = [torch.cuda.Event() for _ in range(2)]

        def analysis(xc, b, stream=None):
            if fused:
                st.encode_chunk(xc, out=b, stream=stream)
            else:
                st.transform_chunk(xc, out=b[0], stream=stream)

        def chain():
            st.reset()
            for i, xc in enumerate(chunks):
                analysis(xc, bufs[0])
                st.inverse_chunk(bufs[0][0], out=xo[0])

        def pipelined():
            st.reset()
            torch.cuda.synchronize()
            for i, xc in enumerate(chunks):
                j = i & 1
                if i >= 2:
                    s1.wait_event(done_s[j])          # synthesis of chunk i-2 has read this buffer
                analysis(xc, bufs[j], stream=s1)
                done_a[j].record(s1)
                s2.wait_event(done_a[j])
                st.inverse_chunk(bufs[j][0], out=xo[j], stream=s2)
                done_s[j].record(s2)
            torch.cuda.synchronize()

        def wall(fn, reps=3):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts))

        def one_call():          # ac_stream_run: issued from C; one clip: analysis of chunk i+1 + synthesis of chunk i per launch
            st.reset()
            st.run(chunks if Bs > 1 else xs[:, :len(chunks) * k * N], k, masking=fused)

        def one_call_graph():    # the same call captured once into a HIP graph and replayed (StreamingMDCT.run(graph=True))
            st.reset()
            st.run(chunks if Bs > 1 else xs[:, :len(chunks) * k * N], k, masking=fused, graph=True)

        fr = Bs * 2 * k * len(chunks)
        row = {"chunks": len(chunks)}
        for name, fn in (("chain_one_stream", chain), ("pipelined_two_streams", pipelined), ("ac_stream_run", one_call),
                         ("ac_stream_run_graph_replay", one_call_graph)):
            dt = wall(fn)
            row[name] = {"ms": dt * 1e3, "frames_per_s": fr / dt, "us_per_chunk": dt / len(chunks) * 1e6,
                         "x_real_time": (k * len(chunks) * N / 48000.0) / dt,
                         "GBs": fr * (20484 if fused else 16384) / dt / 1e9}
        lat = []
        for _ in range(21):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            analysis(chunks[0], bufs[0])
            st.inverse_chunk(bufs[0][0], out=xo[0])
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        row["chunk_latency_us_host_synchronised"] = float(np.median(lat)) * 1e6
        st.close()
        return row

    out["configs[4]"] = {
        "workload": "10 min of 48 kHz stereo (28125 blocks) in chunks of 256 blocks; analysis (+ masking model) and synthesis per chunk",
        "bytes_per_frame": {"transform+inverse": 2 * 8 * N, "encode+inverse": 12 * N + 4 + 8 * N},
        "one_clip_transform": stream_case(1, 28125, False),
        "one_clip_encode": stream_case(1, 28125, True),
        "batch64_encode": dict(stream_case(64, 2048, True), workload="64 concurrent stereo streams, 2048 blocks each"),
    }
    return out


def main():
    args = parse_args()
    if args.gpus < 1:
        sys.exit("--gpus must be >= 1")
    if args.steps < 1:
        sys.exit("--steps must be >= 1")
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)
    in_torchrun = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    force_dist = args.dist in ("nccl", "gloo") or os.environ.get("AC_BENCH_FORCE_DIST", "") not in ("", "0")
    if not in_torchrun and (args.gpus > 1 or force_dist or args.dry_run_launch):
        sys.exit(launch_ranks(args))           # nothing in this process has touched the GPU; the ranks are children

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE is %d (launch with `python bench.py --gpus %d`, or with "
                 "torch.distributed.run --nproc-per-node %d)" % (args.gpus, world, args.gpus, args.gpus))
    # a process group whenever the ranks were started by torch.distributed.run -- ONE rank included (--dist none opts
    # out): RCCL ("nccl") carries the barrier, the max-over-ranks time and the scalar reductions on the device;
    # AC_BENCH_BACKEND=gloo rehearses the multi-rank path on a box with fewer GPUs than ranks (ranks then share devices)
    use_dist = in_torchrun and args.dist != "none"
    backend = (os.environ.get("AC_BENCH_BACKEND") or (args.dist if args.dist in ("nccl", "gloo") else "nccl")) if use_dist else None
    cpu = smi = None
    if world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline()                   # before this process initialises the GPU
    if rank == 0 and not args.no_smi:
        smi = SmiSampler()                     # child process, started before this process initialises the GPU

    import numpy as np
    import torch
    import audiocodec_amd
    from audiocodec_amd import dist as acd

    ndev = torch.cuda.device_count()           # (does not initialise the GPU)
    if ndev <= 0:
        sys.exit("bench.py needs the MI355X")
    if backend == "nccl" and ndev < world:     # before any process group exists: a rank without its own device cannot join
        sys.exit("bench.py: %d ranks over RCCL need %d devices, this box has %d" % (world, world, ndev))
    rank, world, local_rank = acd.init_process_group(backend, force=use_dist)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs the MI355X")
    dev = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(dev)

    B = args.clips if args.clips > 0 else (CLIPS_1GPU if world == 1 else CLIPS_PER_RANK)
    K, C = args.blocks, 2
    codec = audiocodec_amd.AudioCodec(48000, N)
    if not (codec.mdct.is_fast(dev) and codec.psy.is_fast(dev)):
        sys.exit("bench.py: wave-level kernels not selected")
    spreading = codec.psy.plan_spreading(dev)
    x = make_clips(torch, dev, rank * B, B, K)
    X = torch.empty((B, K + 1, N, C), device=dev, dtype=torch.float32)
    t = torch.empty((B, K + 1, 1, C), device=dev, dtype=torch.float32)
    thr = torch.empty((B, K + 1, N, C), device=dev, dtype=torch.float32)
    xh = torch.empty((B, (K + 2) * N, C), device=dev, dtype=torch.float32)

    def barrier():
        acd.reduce_scalars([0.0], "sum", device=dev)      # RCCL all-reduce of one scalar

    # cold start, for the record: `warmup` + `steps` steps straight from an idle device (what the same command measures
    # without the settle phase); not the headline
    cold = None
    if args.settle_ms > 0:
        run_steps(torch, codec, x, X, t, thr, xh, 2)      # first-launch costs (module load) are not part of it
        torch.cuda.synchronize()
        time.sleep(0.25)
        run_steps(torch, codec, x, X, t, thr, xh, args.warmup)
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        ce, cd = run_steps(torch, codec, x, X, t, thr, xh, args.steps, timed=True)
        cel = time.perf_counter() - c0
        cold = {"value_rank0": B * C * K * args.steps / cel, "ms_per_step": cel / args.steps * 1e3,
                "encode_ms": float(np.mean(ce)), "decode_ms": float(np.mean(cd)),
                "encode_ms_per_step": [round(v, 4) for v in ce[:32]],
                "note": "the same %d + %d steps started 250 ms after the device went idle, no settle phase" % (args.warmup, args.steps)}
    # the step on caller-owned plain tensors (encode_into / decode_into: what a C-ABI caller with its own buffers gets), beside
    # the headline
    co_el, co_enc, co_dec, _, _, _ = timed_loop(torch, codec, x, X, t, thr, xh, args.steps, args.warmup, None, args.settle_ms)
    err_co = float((xh[:, N:-N] - x).abs().max()) if K > 0 else 0.0
    # THE HEADLINE: the step through the API of the reference's classes (the library allocates what it returns)
    elapsed, enc_all, dec_all, w0, w1, settled, outs = timed_loop_api(torch, codec, x, args.steps, args.warmup, barrier,
                                                                     args.settle_ms)
    X, t, thr, xh = outs
    elapsed_max, = acd.reduce_scalars([elapsed], "max", device=dev)   # also the closing barrier
    # parity guard on the benchmark data itself + the cross-rank aggregates of SURVEY 8(e): frames, checksums of
    # X / thr / PCM (float64 sums), maximum round-trip error (<= 1 LSB of int16)
    err = float((xh[:, N:-N] - x).abs().max()) if K > 0 else 0.0
    frames_rank = B * C * K
    sums = acd.reduce_scalars([frames_rank, float(X.sum(dtype=torch.float64)), float(thr.sum(dtype=torch.float64)),
                               float(xh.sum(dtype=torch.float64)), float(t.sum(dtype=torch.float64))], "sum", device=dev)
    err_max, = acd.reduce_scalars([err], "max", device=dev)
    if err_max > 1.0 / 32768.0:
        sys.exit("bench.py: round trip error %g exceeds 1 LSB of int16" % err_max)
    dumped = None
    if rank == 0 and args.dump_outputs:      # outside the timed region; before the side measurements free these tensors
        dumped = dump_outputs(np, torch, args.dump_outputs,
                              {"encode_X": X, "encode_tonality": t, "encode_threshold": thr, "decode_pcm": xh})
    ranks_seen = torch.distributed.get_world_size() if use_dist else world
    backend_seen = torch.distributed.get_backend() if use_dist else None
    enc_ms, dec_ms = float(np.mean(enc_all)), float(np.mean(dec_all))
    frames_total = int(sums[0]) * args.steps
    value = frames_total / elapsed_max

    if rank == 0:
        tr = measured_traffic() if (B, K) == (256, 468) else None
        traffic = tr[0]["encode"]["hbm_bytes_per_launch"] if tr else None
        enc_gbs = ENC_BYTES * frames_rank / (enc_ms * 1e-3) / 1e9
        dec_gbs = DEC_BYTES * frames_rank / (dec_ms * 1e-3) / 1e9
        cfg = "configs[1]" if world == 1 else "configs[2] rank share"
        side = {
            "kernels": {"encode_ms": enc_ms, "encode_GBs": enc_gbs, "decode_ms": dec_ms, "decode_GBs": dec_gbs,
                        "encode_ms_median": float(np.median(enc_all)), "encode_ms_min": float(np.min(enc_all)),
                        "decode_ms_median": float(np.median(dec_all)), "decode_ms_min": float(np.min(dec_all)),
                        "encode_ms_per_step": [round(v, 4) for v in enc_all[:64]],
                        "decode_ms_per_step": [round(v, 4) for v in dec_all[:64]],
                        # the step against the spec peak, against the measured streaming-copy rate, and the
                        # read-only share
                        "step_frac_of_hbm_peak": (ENC_BYTES + DEC_BYTES) * (value / world) / (HBM_PEAK_GBS * 1e9),
                        "step_frac_of_achievable_6290_GBs": (ENC_BYTES + DEC_BYTES) * (value / world) / 6.29e12,
                        "step_read_share_of_hbm_peak": 2 * 4 * N * (value / world) / (HBM_PEAK_GBS * 1e9)},
            "workload": "BASELINE %s: batch=%d stereo 48 kHz clips per GPU, N=1024, K=%d blocks (%.1f s), fused MDCT+tonality+"
                        "masking encode then IMDCT decode through codec.encode() / decode() (the library allocates its results, as "
                        "the reference's API does); clips split across ranks, no data-path collective" % (cfg, B, K, K * N / 48000.0),
        }
        if cold is not None:
            side["cold_start"] = cold
        if dumped is not None:
            side["dump_outputs"] = dumped
        if smi is not None:
            pr = torch.cuda.get_device_properties(dev)
            side["gpu_state"] = smi.finish(w0, w1, "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id))
        flat = {"caller_owned_value": frames_rank * args.steps / co_el, "caller_owned_encode_ms": float(np.mean(co_enc)),
                "caller_owned_decode_ms": float(np.mean(co_dec))}
        side["caller_owned"] = {"value_rank0": flat["caller_owned_value"], "ms_per_step": co_el / args.steps * 1e3,
                                "encode_ms_per_step": [round(v, 4) for v in co_enc[:64]], "round_trip_max_abs_err": err_co,
                                "note": "the same step on caller-owned plain torch allocations (encode_into / decode_into)"}
        rep = getattr(codec, "placement_report", None)
        side["placement"] = rep(dev) if callable(rep) else None
        if not args.no_workspace and world == 1:
            # the same step on tensors placed by audiocodec_amd.Workspace (DESIGN_LOG.md 9a), beside the headline
            try:
                del X, t, thr, xh, outs
                ws = audiocodec_amd.Workspace(codec, B, K, C, device=dev)
                ws.x.copy_(x)
                el, e2, d2, _, _, _ = timed_loop(torch, codec, ws.x, ws.X, ws.t, ws.thr, ws.xh, args.steps, args.warmup,
                                                 settle_ms=args.settle_ms)
                side["workspace_placed"] = {"value": frames_rank * args.steps / el, "ms_per_step": el / args.steps * 1e3,
                                            "encode_ms": float(np.mean(e2)), "decode_ms": float(np.mean(d2)),
                                            "placement": ws.report}
                flat["workspace_value"] = side["workspace_placed"]["value"]
                flat["workspace_encode_ms"] = side["workspace_placed"]["encode_ms"]
                del ws
            except Exception as e:
                side["workspace_placed"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if cpu is not None:
            side["cpu_baseline"] = cpu
        if world == 1 and not args.no_other_configs:
            del x
            try:
                oc = other_configs(torch, np, audiocodec_amd, dev, min(args.steps, 50), args.warmup, args.settle_ms)
                side["other_configs"] = oc
                flat["f32_spreading_value"] = oc["f32_spreading"]["value"]
                flat["f32_spreading_encode_ms"] = oc["f32_spreading"]["encode_ms"]
                flat["k46_value"] = oc["k46_cache_resident"]["value"]
                flat["configs3_encode_ms"] = oc["configs[3]"]["spreading"]["bf16x2_mfma"]["encode_ms"]
                flat["configs3_decode_ms"] = oc["configs[3]"]["decode_ms"]
                flat["n960_analysis_GBs"] = oc["lds_fft_tier"]["filters_n"]["960"]["analysis_GBs"]
                flat["n960_synthesis_GBs"] = oc["lds_fft_tier"]["filters_n"]["960"]["synthesis_GBs"]
                flat["n4096_analysis_GBs"] = oc["lds_fft_tier"]["filters_n"]["4096"]["analysis_GBs"]
                flat["n4096_synthesis_GBs"] = oc["lds_fft_tier"]["filters_n"]["4096"]["synthesis_GBs"]
                flat["configs4_one_clip_frames_per_s"] = oc["configs[4]"]["one_clip_encode"]["ac_stream_run_graph_replay"]["frames_per_s"]
                flat["configs4_batch64_frames_per_s"] = oc["configs[4]"]["batch64_encode"]["ac_stream_run_graph_replay"]["frames_per_s"]
            except Exception as e:   # side measurements must never cost the headline line
                side["other_configs"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if cold is not None:
            flat["cold_start_value"] = cold["value_rank0"]
            flat["cold_start_encode_ms"] = cold["encode_ms"]
        # ---- the contract line: LAST line of stdout, < 2 KB, flat scalars for the side figures (their detail is in the
        # "bench_side" line printed before it)
        out = {
            "metric": "MDCT frames/s (48 kHz, N=1024) encode+decode",
            "value": value, "unit": "frames/s", "n_gpus": ranks_seen, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed_max / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE %s: %d stereo 48 kHz clips/GPU x %d blocks, N=1024, codec.encode() + decode() (library-"
                                   "allocated results)" % (cfg, B, K),
                       "clips_per_gpu": B, "clips_total": B * world, "channels": C, "blocks": K, "filters_n": N,
                       "sharding": "clips", "backend": backend_seen, "devices": min(world, ndev)},
            "roofline": {"bound": "hbm", "kernel": "k_fwd_fast<8,0,true,4,0,%d> fused encode, %s spreading"
                                   % (audiocodec_amd.PsychoacousticModel.SPREADING[spreading], spreading),
                         "achieved": enc_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": enc_gbs / HBM_PEAK_GBS,
                         "traffic": traffic,
                         "traffic_source": ("%s (committed PMC pass, not this run)" % tr[1]) if tr else None,
                         "bytes_per_frame": ENC_BYTES, "frames_per_launch": frames_rank, "avg_launch_ms": enc_ms},
            "cpu_baseline": ({k: cpu[k] for k in ("value", "unit", "cores", "kind", "cores_bound", "host_cpus", "reference_shaped_value",
                                                  "reference_shaped_cores")} if cpu else None),
            "timed_region_s": elapsed_max, "settle_ms": args.settle_ms, "settle_steps": settled,
            "encode_ms": enc_ms, "decode_ms": dec_ms,
            "reduced_over_ranks": {"frames_per_step": int(sums[0]), "checksum_X": sums[1], "checksum_thr": sums[2],
                                   "checksum_pcm": sums[3], "checksum_tonality": sums[4],
                                   "round_trip_max_abs_err": err_max},
        }
        if cpu:
            out["cpu_baseline"]["sample"] = ("%d procs x 12 s of B=2 K=46 stereo encode+decode, numpy oracle (closed form: value; "
                                              "reference-shaped dense ops, 8 s: reference_shaped_value)" % cpu["processes"])
        out.update(flat)

        def trim(o):   # seven significant digits are plenty for a rate or a time (checksums keep all of theirs)
            if isinstance(o, dict):
                return {k: (v if k.startswith("checksum") else trim(v)) for k, v in o.items()}
            return float("%.7g" % o) if isinstance(o, float) else o
        out = trim(out)
        out["roofline"]["frac"] = out["roofline"]["achieved"] / out["roofline"]["peak"]   # (consistent after the rounding)
        side_line = json.dumps({"bench_side": side})
        if args.side_json:
            with open(args.side_json, "w") as f:
                f.write(side_line + "\n")
        print(side_line, flush=True)
        line = json.dumps(out, separators=(",", ":"))
        for k in reversed(list(flat)):   # never lose the line to its own size: shed side scalars first (they stay in bench_side)
            if len(line) < 2000:
                break
            out.pop(k, None)
            line = json.dumps(out, separators=(",", ":"))
        print(line, flush=True)
    if use_dist:
        if backend_seen == "nccl":
            torch.distributed.barrier(device_ids=[dev.index])
        else:
            torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

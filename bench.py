#!/usr/bin/env python
"""bench.py -- end-to-end queries/sec (embed + retrieve + register) of the CORSAIR hot path on MI355X.

Workloads (BASELINE.json `configs`), selected with --workload:

  chair  (default, configs[1]) Scan2CAD-chair-sized synthetic evaluation: catalog of 652 CAD clouds, query
         pool 993, labels 650 x sym 1 + 2 x sym 4, 10 000 points @ voxel 0.03.
  table  (configs[2]) Scan2CAD-table-sized: catalog 830, query pool 291, symmetry labels with the
         histogram of configs/04379243_scan2cad_rot_sym_label.txt (233 x 1, 422 x 2, 7 x 3, 128 x 4,
         40 x 12): 72 % of the CADs take the K = 4 + mirror path (9 RANSACs per query instead of 3).
  stress (configs[4]) batch-64 sparse ResUNet forward on 15 000-point clouds @ 2 cm voxels + descriptor
         top-10 against a 10^6 catalog; a step = 1024 clouds (16 batches) + their share of the
         10^6 x 10^6 top-10 (10 240 queries).

chair / table: a step = one batch of 32 queries through GPU voxelise -> sparse ResUNet forward -> global
descriptor -> exact top-1 against the catalog descriptors -> symmetry-aided registration against the
top-1 CAD (feature 5-NN, part cut, K(+4) part hypotheses, batched RANSAC 100 000 x ransac_n 10,
Chamfer).  Random-init ResUNetBN2C + embedding weights (the reference checkpoints / ScanNet data are
not available).  Raw query clouds and the embedded catalog are resident in HBM before the timed region.

--gpus N: one process per GPU (torch.distributed, backend "nccl" = RCCL).  Under torchrun
(WORLD_SIZE set) this process is one rank; started plainly with --gpus N > 1 it launches the N ranks as
a child `python -m torch.distributed.run` BEFORE anything touches the GPU and exits with its code.
configs[3] is `--gpus 8 --workload chair` / `table`: the catalog is embedded in voxel-count-balanced
shards and all-gathered once (setup, reported as catalog_embed_s); queries are sharded with a fixed
per-GPU count ("weak"); the timed region contains no collective.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps of the pass that gives `value` and prints the line.  --full adds what
the line carried before that split: the sequential pass next to the batches-in-flight pass (results compared), the
roofline and per-kernel figures, the stand-alone prefilter probe, the table / stress / converging legs of a chair run
and the CPU baseline.  --dump-outputs DIR writes the arrays the last timed step returned as DIR/<name>.npy (rank 0).
"""
import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_PEAK_TFLOPS = 157.3   # MI355X f32: matrix (v_mfma_f32_32x32x2_f32) == vector peak (MI355X_MICROARCH.md)
F64_PEAK_TFLOPS = 78.6
F16_PEAK_TFLOPS = 2516.6  # dense f16/bf16 MFMA: 1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz (16x the f32 matrix rate)
BATCH = 32
# the arithmetic types the path computes in (the contract's `dtype`: not a precision claim).  Nothing is computed at lower
# precision than the reference: the f16 matrix-core stages are proven upper bounds / shortlists whose survivors are
# recounted or re-scored in f64
DTYPE_LABEL = {"registration": "f32 sparse conv + embedding / f64 RANSAC, k-NN, Chamfer, top-k / f16 MFMA bounds and shortlists "
                               "(survivors recounted in f64)",
               "stress": "f32 sparse conv + embedding / f64 top-k re-score / f16 MFMA shortlist", "dry": "none"}
# the full 32-query C1 shape on the CPU port (`--cpu-sample 32 --cpu-problems 100000`), measured once per round
# on a GPU box's host cores and printed next to the bounded sample of every run
FULL_SHAPE_CPU = {
    "chair": {"value": 0.171, "unit": "queries/s", "cores": 16, "seconds": 187.5, "date": "round 4", "commit": "f255a11",
              "file": "profiles/r4t_chair_cpu32_line.json"},
}

# label -> count; table: histogram of the reference's configs/04379243_scan2cad_rot_sym_label.txt
# (SURVEY 2 #28), chair: configs/03001627_scan2cad_rot_sym_label.txt
SYM_HISTOGRAM = {"chair": {1: 650, 4: 2}, "table": {1: 233, 2: 422, 3: 7, 4: 128, 12: 40}}
QUERY_POOL = {"chair": 993, "table": 291}
FAMILIES = ("conv", "ransac_eval", "ransac_pre", "ransac_hyp", "knn", "chamfer", "topk", "symcut", "kmap")
KERNEL_OF = {"conv": "k_conv_dma", "ransac_eval": "k_ransac_count", "ransac_pre": "k_ransac_prefilter",
             "knn": "k_knn_f16", "chamfer": "k_chamfer_f16", "topk": "k_topk_f16"}
# (round 5: the Chamfer ranking runs on the f16 matrix cores -- one K = 16 MFMA per 32 x 32 pairs --, priced against that peak)
PEAK_OF = {"knn": F16_PEAK_TFLOPS, "chamfer": F16_PEAK_TFLOPS, "ransac_pre": F16_PEAK_TFLOPS,
           "topk": F16_PEAK_TFLOPS}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=("chair", "table", "stress", "dry"), default="chair",
                    help="dry: NO kernels, NO GPU -- the launcher / rank layout / collectives / one-JSON-line plumbing alone "
                         "(tests/test_bench_launch_cpu.py runs it with 8 CPU ranks); never a measurement")
    ap.add_argument("--allow-gloo", action="store_true",
                    help="N > 1: if the RCCL communicator does not come up, run the exchange over gloo instead of "
                         "failing (every rank must agree; the JSON line then says dist.backend = gloo)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=6,
                    help="most queries in the CPU baseline sample (SURVEY 8d's full shape: 32)")
    ap.add_argument("--cpu-problems", type=int, default=12,
                    help="the CPU sample stops once it has run this many RANSAC problems (~1.9 s each on 16 cores)")
    ap.add_argument("--cpu-catalog", type=int, default=64,
                    help="catalog subset the CPU baseline retrieves against (SURVEY 8d: 64)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default, the driver's contract): 32 queries per rank and step.  strong: chair / table only, one "
                         "step = one WHOLE evaluation of the query pool (993 / 291) spread over the ranks, results gathered "
                         "to one result set (configs[3] as time to solution)")
    ap.add_argument("--queries", type=int, default=0, help="--scaling strong: size of the query pool (default: the category's)")
    ap.add_argument("--catalog", type=int, default=0, help="catalog size (default: the workload's)")
    ap.add_argument("--desc-dim", type=int, default=256, help="stress: descriptor width (256 or 512)")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="query batches in flight in the timed region (host threads x HIP streams)")
    ap.add_argument("--no-solo-probe", action="store_true",
                    help="skip the extra pass that times the dominant kernel without concurrent work")
    ap.add_argument("--no-extra-workloads", action="store_true",
                    help="chair, 1 GPU: skip the short table (configs[2]) and stress (configs[4]) legs reported as `workloads`")
    ap.add_argument("--sequential-value", action="store_true",
                    help="report the one-batch-at-a-time pass as `value` even when the three-batches-in-flight pass ran")
    ap.add_argument("--embed-group", type=int, default=4,
                    help="N consecutive steps of the chair / table workload share one forward of the network "
                         "(N x 32 clouds; retrieval and registration stay per step of 32 queries); 1: one forward per step")
    ap.add_argument("--in-flight", type=int, default=3,
                    help="batches in flight in the pass that gives `value` (host threads x HIP streams; default 3); 0: the "
                         "depth in 3..6 that leaves the K timed steps the least ragged last round (experiment: faster on "
                         "average, but one run in four shows a 0.5-s stall somewhere -- DESIGN 7)")
    ap.add_argument("--no-overlap-probe", action="store_true",
                    help="skip the extra pass with three batches in flight reported as `batches_in_flight`")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline as well: the sequential pass next to the batches-in-flight pass "
                         "(results compared), roofline / per-kernel figures, the stand-alone prefilter probe, the table / "
                         "stress / converging legs and the CPU baseline.  Without it a run times only the pass that gives "
                         "`value`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0) as DIR/<name>.npy, "
                         "float32 / float64")
    return ap.parse_args()


def visible_device_count():
    """GPUs this process may use, WITHOUT touching HIP (the launcher parent must stay a plain process: its
    ranks start as a child, never by exec): the KFD topology lists one node per device, *_VISIBLE_DEVICES
    narrows it.  Falls back to torch only if sysfs is unreadable."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    try:
        n = 0
        root = "/sys/class/kfd/kfd/topology/nodes"
        for node in os.listdir(root):
            with open(os.path.join(root, node, "properties")) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:      # CPU nodes have no SIMDs
                n += 1
        # a container may SEE the host's whole topology but be allowed to open only some render nodes:
        # count the devices this process can actually open
        try:
            nodes = [f for f in os.listdir("/dev/dri") if f.startswith("renderD")]
            usable = sum(os.access(os.path.join("/dev/dri", f), os.R_OK | os.W_OK) for f in nodes)
            if nodes and usable < n:
                n = usable
        except OSError:
            pass
        return n
    except OSError:
        import torch

        return torch.cuda.device_count()


def maybe_self_launch(args):
    """`python bench.py --gpus N` without torchrun: start the N ranks as a CHILD process (never an exec,
    and before this process has made any HIP call) and leave with its return code."""
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != args.gpus:
            sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%s; refusing to report a mislabelled run\n"
                             % (args.gpus, ws))
            sys.exit(2)
        return
    if args.gpus <= 1:
        return
    env = dict(os.environ)
    n_dev = visible_device_count()
    if n_dev < args.gpus and "CORSAIR_DIST_BACKEND" not in env:
        # rehearsal on a box with fewer devices than ranks: ranks share devices, RCCL cannot (it needs
        # one device per rank), so the exchange runs over gloo; the JSON line says so
        sys.stderr.write("[bench] %d ranks on %d visible device(s): ranks share devices, backend gloo\n"
                         % (args.gpus, n_dev))
        env["CORSAIR_DIST_BACKEND"] = "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


class GroupDist:
    """The handful of torch.distributed calls the sharded path makes, bound to ONE process group (None = the default
    group): corsair_amd.sharding takes any object with these methods."""

    def __init__(self, dist, group):
        self._d, self._g = dist, group
        self.ReduceOp = dist.ReduceOp

    def get_backend(self):
        return self._d.get_backend(self._g)

    def all_gather(self, out, t):
        return self._d.all_gather(out, t, group=self._g)

    def all_gather_into_tensor(self, out, t):
        return self._d.all_gather_into_tensor(out, t, group=self._g)

    def all_reduce(self, t, op=None):
        return self._d.all_reduce(t, op=self._d.ReduceOp.SUM if op is None else op, group=self._g)

    def barrier(self):
        return self._d.barrier(group=self._g)

    def destroy_process_group(self):
        return self._d.destroy_process_group()


class Ctx:
    """What a workload needs from the process: rank layout, device, the one dist handle, logging."""

    def __init__(self, args):
        import torch

        from corsair_amd import _lib

        self.args = args
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.dry = args.workload == "dry"
        # one process per GPU; CORSAIR_DIST_BACKEND=gloo lets several ranks share one GPU to rehearse the
        # N > 1 code path on a single-GPU box (RCCL needs distinct devices)
        self.backend = os.environ.get("CORSAIR_DIST_BACKEND", "nccl")
        if self.dry:
            self.backend, self.n_devices, self.dev_index, self.dev = "gloo", 0, 0, torch.device("cpu")
        else:
            _lib.require_gpu()
            self.n_devices = torch.cuda.device_count()
            self.dev_index = local_rank % self.n_devices
            torch.cuda.set_device(self.dev_index)
            self.dev = torch.device("cuda", self.dev_index)
        self.dist = None
        if self.world > 1:
            import torch.distributed as dist
            from datetime import timedelta

            # The DEFAULT group is always gloo (control plane: it comes up wherever TCP does); RCCL is a second group
            # the data collectives run on.  Whether RCCL is usable is agreed on over gloo BEFORE anything depends on it
            # (no second TCPStore on MASTER_PORT + 1, no rank left blocking in an RCCL collective while its
            # peer has already given up -- the RCCL group has its own, finite timeout).
            dist.init_process_group("gloo")
            group, err = None, None

            def all_ranks_ok(e):
                """gloo MIN all-reduce: does EVERY rank report success for the stage just done?"""
                ok = torch.tensor([0 if e is not None else 1], dtype=torch.int32)
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                return int(ok) == 1

            if self.backend == "nccl":
                # Stage 1 (local, no peer involved): the device answers.  Stage 2: the RCCL group object exists.  Both are
                # agreed on over gloo BEFORE the first RCCL collective (a rank whose peer never joins the
                # communicator would otherwise sit in the probe until the RCCL timeout and be aborted by the watchdog,
                # never reaching the documented exit).  Stage 3: the probe collective itself.
                try:
                    torch.zeros(1, device=self.dev).add_(1).item()
                except Exception as e:                      # noqa: BLE001 (reported below, with the rank)
                    err = e
                ok = all_ranks_ok(err)
                if ok:
                    try:
                        # (the group's timeout bounds how long a healthy rank waits in the probe for a peer whose RCCL did not
                        # come up -- and every later collective: ranks reach the catalog all-gather within seconds of each other)
                        group = dist.new_group(backend="nccl", timeout=timedelta(seconds=300), device_id=self.dev)
                    except Exception as e:                  # noqa: BLE001
                        err = e
                    ok = all_ranks_ok(err)
                if ok:
                    try:
                        probe = torch.ones(1, device=self.dev)
                        dist.all_reduce(probe, group=group)     # first collective: the communicator really comes up
                        torch.cuda.synchronize()
                        if int(probe.item()) != self.world:
                            raise RuntimeError("RCCL probe all-reduce returned %r, expected %d" % (probe.item(), self.world))
                    except Exception as e:                  # noqa: BLE001
                        err = e
                    ok = all_ranks_ok(err)
                if not ok:
                    # RCCL failing to come up is an ERROR (exit non-zero with the reason): a scaling run that quietly
                    # measured gloo would be worse than none.  --allow-gloo turns it into a gloo run on ALL ranks.
                    if not args.allow_gloo:
                        sys.stderr.write("[bench] rank %d: RCCL unusable on at least one rank (here: %s)\n[bench] refusing to "
                                         "fall back to gloo silently (pass --allow-gloo to measure over gloo)\n"
                                         % (self.rank, err))
                        sys.exit(3)
                    sys.stderr.write("[bench] rank %d: RCCL unusable on at least one rank (here: %s); --allow-gloo: all "
                                     "ranks use gloo\n" % (self.rank, err))
                    self.backend, group = "gloo", None
            self.dist = GroupDist(dist, group)

    def log(self, msg):
        if self.rank == 0:
            print("[bench] " + msg, file=sys.stderr, flush=True)

    def barrier(self):
        import torch

        if self.dist is not None:
            self.dist.barrier()
        self.sync()

    def sync(self):
        if not self.dry:
            import torch

            torch.cuda.synchronize()

    def reduce_max(self, vals):
        """max over ranks of a list of floats (host list in, host list out)."""
        import torch

        if self.dist is None:
            return list(vals)
        t = torch.tensor(vals, device=self.dev if self.backend == "nccl" else "cpu", dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    def gather_floats(self, vals):
        """[world, len(vals)] array of every rank's values (on every rank)."""
        import torch

        if self.dist is None:
            return np.asarray([vals], dtype=np.float64)
        t = torch.tensor(vals, device=self.dev if self.backend == "nccl" else "cpu", dtype=torch.float64)
        out = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return torch.stack(out).cpu().numpy()


def sym_labels(kind, n):
    """Per-CAD symmetry labels with the label histogram of the reference's label file, dealt to catalog
    ids by a seeded permutation (scaled when --catalog differs from the real size)."""
    hist = SYM_HISTOGRAM[kind]
    total = sum(hist.values())
    labels = np.concatenate([np.full(c, l, np.int32) for l, c in sorted(hist.items())])
    if n != total:
        labels = labels[(np.arange(n) * total) // max(n, 1)] if n < total else np.resize(labels, n)
    rng = np.random.Generator(np.random.Philox(key=0x5A1B, counter=n))
    return labels[rng.permutation(n)]


# =====================================================================================================
class RegistrationWorkload:
    """configs[1] (chair) / configs[2] (table): embed + retrieve + register, 32 queries per step."""

    def __init__(self, ctx, kind, converging=False):
        from corsair_amd import harness, synth

        self.ctx, self.kind = ctx, kind
        # converging = True (the `converging` leg of the default line): the same shapes and the same forward
        # of the network, but what retrieval and registration READ is pose-invariant -- voxel features = the voxel's CAD-frame
        # coordinates zero-padded to 16-d (feature 5-NN = spatial 5-NN in the CAD frame), descriptors = the CAD's seeded unit
        # vector plus noise -- because random-init weights carry no signal.  Retrieval then finds the right CAD, RANSAC leaves
        # through its confidence bound, and the line can show that the batched path recovers poses at bench scale
        # (evaluation.py:334-383's metrics) instead of only timing the 100 000-iteration worst case.
        self.converging = converging
        self.cfg = harness.Config()
        self.C = ctx.args.catalog or sum(SYM_HISTOGRAM[kind].values())
        self.pool = QUERY_POOL[kind]
        self.sd, self.emb = synth.make_state_dicts(self.cfg.random_seed)
        self.pipe = harness.Pipeline(self.sd, self.emb, device=ctx.dev, config=self.cfg)
        self.sym = sym_labels(kind, self.C)
        self.results = []
        self.units_per_step = BATCH
        self.last_step, self.last_out = ctx.args.warmup + ctx.args.steps - 1, None

    def setup(self):
        import torch

        from corsair_amd import backend as B, sharding, synth

        ctx, cfg, C = self.ctx, self.cfg, self.C
        args = ctx.args
        # ---- catalog: voxel-count pre-pass on an interleaved slice, balanced shards, embed, all-gather ----
        t1 = time.time()
        mine = sharding.shard_ids(C, ctx.rank, ctx.world)
        clouds = {c: synth.make_cloud(c, 15000)[: cfg.n_points] for c in mine}
        counts = []
        for i in range(0, len(mine), 64):
            chunk = [clouds[c] for c in mine[i:i + 64]]
            off = np.concatenate([[0], np.cumsum([len(c) for c in chunk])]).tolist()
            _, _, out_off = B.voxelize(torch.from_numpy(np.concatenate(chunk, 0)).to(ctx.dev), off, cfg.voxel_size)
            counts += list(np.diff(out_off))
        vox = sharding.all_gather_counts(ctx.dist, mine, counts, C, ctx.world)
        shards = sharding.balanced_shards(vox, ctx.world)
        self.balance = {"catalog_voxels_max_over_mean_balanced": sharding.imbalance(vox, shards),
                        "catalog_voxels_max_over_mean_interleaved": sharding.imbalance(
                            vox, [sharding.shard_ids(C, r, ctx.world) for r in range(ctx.world)])}
        my_cat = shards[ctx.rank]
        cat_clouds = [clouds[c] if c in clouds else synth.make_cloud(c, 15000)[: cfg.n_points] for c in my_cat]
        torch.cuda.synchronize()
        t2 = time.time()
        cat_local = self.pipe.embed_clouds(cat_clouds)
        torch.cuda.synchronize()
        t3 = time.time()
        # the one exchange of the path: RCCL all-gather of the embedded catalog shards over xGMI
        self.catalog = sharding.gather_catalog(ctx.dist, cat_local, C, ctx.world, shards)
        torch.cuda.synchronize()
        t4 = time.time()
        self.catalog_embed_s = t4 - t2
        per_rank = ctx.gather_floats([t3 - t2, t4 - t3])
        self.balance["catalog_embed_s_per_rank"] = [round(float(v), 4) for v in per_rank[:, 0]]
        self.balance["catalog_all_gather_s"] = round(float(per_rank[:, 1].max()), 4)
        self.balance["catalog_prepass_s"] = round(t2 - t1, 3)

        # ---- this rank's queries: posed re-samplings of catalog clouds (known GT pose) ----------------
        n_b = args.warmup + args.steps
        self.n_q = n_b * BATCH
        self.q_ids = [(ctx.rank * self.n_q + i) % self.pool for i in range(self.n_q)]
        self.q_clouds, self.q_T, self.q_cad = [], [], []
        for q in self.q_ids:
            cad = q % C
            T = synth.random_pose(q, max_trans=0.0)
            pc = synth.make_cloud(cad, 15000)[15000 - cfg.n_points:]
            self.q_clouds.append(synth.apply_pose(pc, T, np.float64))   # apply_transform's f64: quantised in f64
            self.q_T.append(T)
            self.q_cad.append(cad)
        self.q_dev, self.q_off = [], []
        for b in range(n_b):
            chunk = self.q_clouds[b * BATCH:(b + 1) * BATCH]
            self.q_dev.append(torch.from_numpy(np.concatenate(chunk, 0)).to(ctx.dev))
            self.q_off.append(np.concatenate([[0], np.cumsum([len(c) for c in chunk])]).tolist())
        if self.converging:
            from corsair_amd import harness

            # catalog side: CAD-frame coordinates ARE the catalog voxels' origins; one seeded unit descriptor per CAD
            cat = self.catalog
            d = synth.make_descriptors(C, cat.desc.shape[1], seed=0xC0DE)
            self.cad_desc = torch.from_numpy(d).to(ctx.dev)
            self.catalog = harness.EmbeddedSet(torch.nn.functional.pad(cat.origin, (0, 13)), cat.origin, cat.offsets,
                                               self.cad_desc)
            # query side: inverse poses (x_cad = R^T (x - t)) and the noisy copy of the CAD's descriptor, per batch
            rng = np.random.Generator(np.random.Philox(key=0xC0DE, counter=ctx.rank))
            self.q_Rt, self.q_desc = [], []
            for b in range(n_b):
                Ts = np.stack(self.q_T[b * BATCH:(b + 1) * BATCH])
                self.q_Rt.append((torch.from_numpy(Ts[:, :3, :3].astype(np.float32)).to(ctx.dev),
                                  torch.from_numpy(Ts[:, :3, 3].astype(np.float32)).to(ctx.dev)))
                noisy = d[self.q_cad[b * BATCH:(b + 1) * BATCH]] + 0.02 * rng.standard_normal((BATCH, d.shape[1])).astype(np.float32)
                self.q_desc.append(torch.from_numpy(noisy / np.linalg.norm(noisy, axis=1, keepdims=True)).to(ctx.dev))
        ctx.log("setup done: %s catalog %d clouds embedded in %.2fs, %d query batches resident"
                % (self.kind, C, self.catalog_embed_s, n_b))

    def step(self, b):
        self._retrieve_and_register(b, self.pipe.embed_batch(self.q_dev[b], self.q_off[b]))

    def step_group(self, steps):
        """Consecutive steps whose query batches go through ONE forward of the network (a 32-cloud batch
        leaves the stride-4 / 8 layers with fewer workgroups than the chip has CUs).  Each step still retrieves and
        registers its own 32 queries.  Batch composition changes no row -- eval-mode BatchNorm, a convolution row is the
        same fma chain whatever else is in the batch, pooling is per sample -- so the results are those of step() calls
        bit for bit (tests/test_gpu_harness.py::test_bench_grouped_forward_equals_one_forward_per_step)."""
        for b, qs in self.embed_steps(steps).items():
            self._retrieve_and_register(b, qs)

    def embed_steps(self, steps):
        """One forward for the query batches of `steps`; {step: EmbeddedSet (row slices of the shared tensors)}."""
        from corsair_amd import harness

        both = self.pipe.embed_groups([(self.q_dev[b], self.q_off[b]) for b in steps])
        off = both.offsets
        out = {}
        for j, b in enumerate(steps):
            lo = j * BATCH
            r0, r1 = off[lo], off[lo + BATCH]
            out[b] = harness.EmbeddedSet(both.F[r0:r1], both.origin[r0:r1], [o - r0 for o in off[lo:lo + BATCH + 1]],
                                         both.desc[lo:lo + BATCH])
        return out

    def register_step(self, b, qs):
        self._retrieve_and_register(b, qs)

    def _retrieve_and_register(self, b, qs):
        from corsair_amd import _lib, registration

        pipe, catalog, rank, n_q = self.pipe, self.catalog, self.ctx.rank, self.n_q
        if self.converging:
            import torch

            from corsair_amd import harness

            # (inside the timed step: the network's outputs were computed above like in every other leg; what retrieval and
            # registration read is replaced by the pose-invariant stand-ins)
            R, t = self.q_Rt[b]
            counts = torch.as_tensor(np.diff(qs.offsets), device=qs.origin.device)
            seg = torch.repeat_interleave(torch.arange(BATCH, device=qs.origin.device), counts, output_size=qs.origin.shape[0])
            x_cad = torch.einsum("nj,njk->nk", qs.origin - t[seg], R[seg])          # R^T (x - t), row-vector form
            qs = harness.EmbeddedSet(torch.nn.functional.pad(x_cad, (0, 13)), qs.origin, qs.offsets, self.q_desc[b])
        ids = [(2 * (rank * n_q + b * BATCH + i), 2 * (rank * n_q + b * BATCH + i) + 1) for i in range(BATCH)]
        # host work that only needs the voxel counts goes here, while the convolutions are still running
        q_anc = [registration.draw_anchors(qs.offsets[i + 1] - qs.offsets[i], 100, ids[i][0]) for i in range(BATCH)]
        top = _lib.to_host(pipe.retrieve(qs.desc, catalog.desc, 1)[:, 0])[0]
        cads = catalog.gather(top)
        # force_gate: with random-init weights the part-cut acceptance gate (tuned to trained
        # features; sym_ransac_success is True for 993/993 queries in the reference's caches) never
        # passes, which would drop the K symmetric hypotheses -- 2/3 of the registration work -- from
        # the timed region.  The bench accepts the best-balanced anchor so every query runs
        # 1 + K (+4) RANSACs like the reference workload.  Parity tests use the real gate.
        # (the converging leg too: coordinates as features never pass the gate of utils/symmetry.py:232-257 either)
        res = pipe.register(qs, cads, self.sym[top], anchor_ids=ids, force_gate=True, query_anchors=q_anc)
        Tb, Tr, cdb, its = _lib.to_host(res.T_best, res.T_ransac, res.cd_best, res.iters)
        self.results.append((b, top, Tb, Tr, cdb, res.ok, its, res.n_problems))
        if b == self.last_step:     # --dump-outputs: what a caller of the path receives for these 32 queries
            self.last_out = {"query_desc": qs.desc, "top1_cad": top, "T_best": Tb, "cd_best": cdb, "T_ransac": Tr,
                             "cd_ransac": res.cd_ransac, "sym_success": res.ok, "ransac_iters": its}

    def same_results(self, a, b):
        return np.array_equal(a[2], b[2]) and np.array_equal(a[6], b[6])

    def solo_env(self):
        return {"CS_RANSAC_OVERLAP": "0", "CORSAIR_SPLIT_RANSAC": "0"}

    def config(self, steps):
        from corsair_amd import harness

        t_l, r_l, hits, iters_all, nprob = [], [], 0, [], 0
        for b, top, Tb, Tr, cdb, ok, iters, n_problems in self.results:
            for i in range(BATCH):
                qi = b * BATCH + i
                t, r = harness.eval_pose(Tb[i], self.q_T[qi], np.eye(4), int(self.sym[top[i]]))
                t_l.append(t)
                r_l.append(r)
                hits += int(top[i] == self.q_cad[qi])
            iters_all.append(iters)
            nprob += n_problems
        agg = harness.aggregate(r_l, t_l)
        iters_all = np.concatenate(iters_all)
        idx = {"chair": 1, "table": 2}[self.kind]
        hist = ", ".join("%d x sym %d" % (int((self.sym == l).sum()), l) for l in np.unique(self.sym))
        what = ("configs[%d], CONVERGING regime: the same shapes and the same forward, retrieval and registration read "
                "pose-invariant stand-ins (CAD-frame coordinates as voxel features, the CAD's seeded descriptor + noise) so that "
                "retrieval hits and RANSAC leaves through its confidence bound (C=%d, 32 queries/step, 10k pts @ voxel 0.03)"
                % (idx, self.C)) if self.converging else None
        return {"workload": what or "configs[%d]: single-MI355X Scan2CAD %s eval shape (C=%d catalog [%s], query pool %d, "
                            "32 queries/step, 10k pts @ voxel 0.03, ResUNetBN2C+embedding random init, "
                            "top-1 retrieval, sym_pose RANSAC 100000x10)" % (idx, self.kind, self.C, hist, self.pool),
                "queries_per_step": BATCH, "catalog": self.C, "catalog_embed_s": self.catalog_embed_s,
                "ransac_problems_per_query": nprob / (steps * BATCH),
                "ransac_mean_iters": float(iters_all.mean()),
                "ransac_early_exit_share": float((iters_all < self.cfg.ransac_max_iter).mean()),
                "top1_hit_rate": hits / (steps * BATCH),
                "rre_mean_deg": agg["rre_mean_deg"], "rre_5": agg["rre_5"], "rre_15": agg["rre_15"], "rte_010": agg["rte_010"]}

    def extras(self, out):
        import ctypes

        from corsair_amd import _lib

        st = (ctypes.c_uint64 * 5)()
        _lib.load().cs_ransac_prefilter_stats(st, 0)
        out["ransac_prefilter"] = {"survivors": int(st[3]), "hypotheses": int(st[4]),
                                   "note": "hypotheses whose f16 upper bound reached the best count and were "
                                           "recounted exactly / all hypotheses evaluated (whole run incl. warmup)"}
        out["shard_balance"] = self.balance
        ps = (ctypes.c_uint64 * 3)()
        _lib.load().cs_pool_stats(ps)
        out["scratch_pool"] = {"live_blocks": int(ps[0]), "freed_by_a_foreign_thread": int(ps[1])}
        import torch

        ms = torch.cuda.memory_stats()
        out["torch_allocator"] = {"device_mallocs": int(ms.get("num_device_alloc", 0)), "device_frees": int(ms.get("num_device_free", 0)),
                                  "reserved_gb": round(torch.cuda.memory_reserved() / 1e9, 3)}

    def cpu_baseline(self):
        """The CPU oracle (kind "port": the build's restatement of the reference CPU path, OpenMP over
        independent rows / registrations) timed on a bounded sample of the same workload: the first
        `cpu_sample` queries of the first timed step -- embed, retrieve against a `cpu_catalog`-item
        subset of the same catalog descriptors (SURVEY 8d's C1 shape is 32 queries x 64 items) and
        register against the top-1 CAD."""
        from corsair_amd import registration as R
        from oracle import native, post, resunet as oref, sparse as osp

        args, cfg, catalog, sym = self.ctx.args, self.cfg, self.catalog, self.sym
        native.load()
        n = min(args.cpu_sample, BATCH * args.steps)
        nc = min(args.cpu_catalog, self.C)
        first = args.warmup * BATCH
        clouds = self.q_clouds[first:first + n]
        cat_desc = catalog.desc[:nc].cpu().numpy()
        off = catalog.offsets
        cat_F = catalog.F[: off[nc]].cpu().numpy()
        cat_X = catalog.origin[: off[nc]].cpu().numpy()
        t0 = time.time()
        grids, origins = [], []
        for pc in clouds:
            xyz, grid, _ = osp.quantize_cloud(pc, cfg.voxel_size)
            grids.append(grid)
            origins.append(xyz.astype(np.float32))       # narrowed after the selection
        coords = osp.sparse_collate(grids)
        feats = np.ones((coords.shape[0], 1), np.float32)
        out, feat8, maps = oref.resunet_forward(self.sd, coords, feats)
        desc = oref.embedding_forward(self.emb, feat8, maps["c8"][:, 0], n)
        t_embed = time.time() - t0
        rank_, _ = post.retrieval_rank(desc, cat_desc)
        top = rank_[:, 0]
        t_ret = time.time() - t0 - t_embed
        qoff = np.concatenate([[0], np.cumsum([len(g) for g in grids])])
        nprob = done = 0
        for i in range(n):
            if nprob >= args.cpu_problems:     # bounded sample: ~10-30 s of CPU work
                break
            done += 1
            F0, x0 = out[qoff[i]:qoff[i + 1]], origins[i]
            c = int(top[i])
            F1, x1 = cat_F[off[c]:off[c + 1]], cat_X[off[c]:off[c + 1]]
            gq = first + i
            a0 = R.draw_anchors(len(F0), 100, 2 * gq)
            a1 = R.draw_anchors(len(F1), 100, 2 * gq + 1)
            post.sym_pose(F0, x0, F1, x1, int(sym[c]), cfg.k_nn, cfg.max_corr, 0, a0, a1,
                          cfg.ransac_max_iter, cfg.ransac_confidence, force_gate=True)
            nprob += 1 + len(R.part_configs(4 if sym[c] >= 2 else 2, int(sym[c])))
        total = time.time() - t0
        t_reg = total - t_embed - t_ret
        per_query = (t_embed + t_ret) / n + t_reg / max(done, 1)
        return {"value": 1.0 / per_query, "unit": "queries/s", "cores": native.num_threads(),
                "cores_visible": native.cores_visible(), "cgroup_cpu_quota": native.cgroup_cpu_quota(),
                "cores_note": "threads = the box's CPU share (min of affinity, cgroup quota, ORACLE_THREADS default 16: a "
                              "one-GPU box of the pool is entitled to 16 of the CPUs it can see)", "kind": "port",
                "full_shape": FULL_SHAPE_CPU.get("chair" if self.C == 652 else "table"),
                "sample": "queries of the first timed step against a %d-item catalog subset (SURVEY 8d C1 shape "
                          "is 32 x 64; the per-query cost does not depend on the subset size beyond the "
                          "retrieval term, so the rate extrapolates linearly): oracle embed of %d queries "
                          "%.2fs + retrieve %.3fs + sym_pose of the first %d of them %.2fs (%d RANSAC "
                          "problems of 100000 iterations); value = 1 / (embed+retrieve per query + "
                          "sym_pose per query)" % (nc, n, t_embed, t_ret, done, t_reg, nprob)}


# =====================================================================================================
class StrongEvalWorkload:
    """configs[3] as TIME TO SOLUTION (`--scaling strong`): one step = ONE whole evaluation of the category's query pool
    (993 chair / 291 table queries) spread over all ranks -- sharding.run_eval_sharded = evaluation.py:207-441: queries
    dealt out by voxel count, embedded, descriptors all-gathered, retrieval statistics, every rank registers its own
    queries, the nine per-query arrays all-gathered into query order, rank 0 aggregates.  The embedded catalog is
    made (sharded + one all-gather) once before the timed region, like `lib_desc` in the reference; value = Q / step."""
    collective_in_step = True
    scaling = "strong"

    def __init__(self, ctx, kind):
        from corsair_amd import harness, synth

        self.ctx, self.kind = ctx, kind
        self.cfg = harness.Config()
        self.C = ctx.args.catalog or sum(SYM_HISTOGRAM[kind].values())
        self.Q = ctx.args.queries or QUERY_POOL[kind]
        self.sd, self.emb = synth.make_state_dicts(self.cfg.random_seed)
        self.pipe = harness.Pipeline(self.sd, self.emb, device=ctx.dev, config=self.cfg)
        self.sym = sym_labels(kind, self.C)
        self.results = []
        self.units_per_step = self.Q          # of the WHOLE job (all ranks together)
        self.last_step, self.last_out = ctx.args.warmup + ctx.args.steps - 1, None

    def setup(self):
        import torch

        from corsair_amd import sharding, synth

        ctx, cfg, C, Q = self.ctx, self.cfg, self.C, self.Q
        t0 = time.time()
        catalog = [synth.make_cloud(c, 15000)[: cfg.n_points] for c in range(C)]
        self.catalog = sharding.embed_catalog_sharded(self.pipe, ctx.dist, ctx.rank, ctx.world, catalog)
        torch.cuda.synchronize()
        self.catalog_embed_s = time.time() - t0
        self.queries, self.q_T = [], []
        for q in range(Q):
            T = synth.random_pose(q, max_trans=0.0)
            self.queries.append(synth.apply_pose(synth.make_cloud(q % C, 15000)[15000 - cfg.n_points:], T, np.float64))
            self.q_T.append(T)
        self.best_match = np.arange(Q) % C
        rng = np.random.Generator(np.random.Philox(key=0x7AB1E, counter=C))
        t = rng.random((C, C))
        self.table = t + t.T                  # stands in for configs/*_scan2cad.npy (pairwise Chamfer of the CADs)
        np.fill_diagonal(self.table, 0.0)
        self.lib_T = np.stack([np.eye(4)] * C)
        ctx.log("setup done: strong-scaling %s evaluation, catalog %d embedded+gathered in %.2fs, %d queries"
                % (self.kind, C, self.catalog_embed_s, Q))

    def step(self, b):
        from corsair_amd import sharding

        res = sharding.run_eval_sharded(self.pipe, self.ctx.dist, self.ctx.rank, self.ctx.world, self.catalog, self.queries,
                                        self.best_match, self.table, np.stack(self.q_T), self.lib_T, self.sym, self.kind,
                                        True, None, True, None, 3)   # three registration batches in flight per rank
        self.results.append((b, res))
        if b == self.last_step:
            self.last_out = dict(res.per_query)

    def same_results(self, a, b):
        return all(np.array_equal(a[1].per_query[k], b[1].per_query[k]) for k in a[1].per_query)

    def solo_env(self):
        return None

    def config(self, steps):
        res = self.results[-1][1]
        idx = {"chair": 1, "table": 2}[self.kind]
        return {"workload": "configs[3] (strong scaling of configs[%d]): ONE Scan2CAD-%s-shaped evaluation per step -- %d queries "
                            "against a %d-CAD catalog spread over the ranks by voxel count, retrieval statistics, sym_pose "
                            "RANSAC 100000x10, per-query results gathered to one result set (evaluation.py:207-441)"
                            % (idx, self.kind, self.Q, self.C),
                "queries_per_step": self.Q, "catalog": self.C, "catalog_embed_s": self.catalog_embed_s,
                "rre_mean_deg": res.sym["rre_mean_deg"], "rre_15": res.sym["rre_15"],
                "precision_at_M": res.stat["precision"], "sym_success_rate": res.sym_success_rate,
                "all_steps_identical": all(self.same_results(self.results[0], r) for r in self.results[1:])}

    def extras(self, out):
        pass


# =====================================================================================================
class StressWorkload:
    """configs[4]: batch-64 forward on 15k-pt clouds @ 2 cm + top-10 against a 10^6-descriptor catalog.
    One step = 16 forward batches (1024 clouds) + the proportional slice of the 10^6 x 10^6 top-10
    (1024 / 100 000 of 10^6 queries = 10 240 queries)."""
    FWD_BATCH = 64
    BATCHES_PER_STEP = 16
    TOPK_PER_STEP = 10240
    N_UNIQUE = 256
    collective_in_step = True   # world > 1: the catalog-sharded top-k all-gathers queries and candidates

    def __init__(self, ctx):
        from corsair_amd import harness, synth

        self.ctx = ctx
        self.cfg = harness.Config(voxel_size=0.02, n_points=15000, batch_size=self.FWD_BATCH)
        self.sd, self.emb = synth.make_state_dicts(31)
        self.pipe = harness.Pipeline(self.sd, self.emb, device=ctx.dev, config=self.cfg)
        self.C = ctx.args.catalog or 1000000
        self.d = ctx.args.desc_dim
        self.units_per_step = self.FWD_BATCH * self.BATCHES_PER_STEP
        self.results = []
        self.voxels = 0
        self.clouds = 0
        self.last_step, self.last_out = ctx.args.warmup + ctx.args.steps - 1, None

    def setup(self):
        import torch

        from corsair_amd import synth

        ctx = self.ctx
        t0 = time.time()
        base = ctx.rank * self.N_UNIQUE
        clouds = [synth.make_cloud(base + c, 15000) for c in range(self.N_UNIQUE)]
        self.batches = []
        for b in range(0, self.N_UNIQUE, self.FWD_BATCH):
            chunk = clouds[b:b + self.FWD_BATCH]
            self.batches.append((torch.from_numpy(np.concatenate(chunk)).to(ctx.dev),
                                 np.concatenate([[0], np.cumsum([len(c) for c in chunk])]).tolist()))
        self.cloud_sample = clouds[:2]
        # descriptors: Philox standard normal, row-normalised; generated in slabs.  N > 1: every rank
        # holds ONE contiguous shard of the catalog (C / N rows); the queries travel (sharding.sharded_topk)
        from corsair_amd import sharding

        self.shard = sharding.catalog_shard(self.C, ctx.rank, ctx.world)
        first, last = self.shard
        self.x = torch.empty((last - first, self.d), dtype=torch.float32, device=ctx.dev)
        for i, s in enumerate(range(0, self.C, 131072)):
            n = min(131072, self.C - s)
            a, b = max(s, first), min(s + n, last)
            if a < b:
                slab = synth.make_descriptors(n, self.d, seed=4321 + i)
                self.x[a - first:b - first] = torch.from_numpy(slab[a - s:b - s]).to(ctx.dev)
        # the library is fixed for the run: its matrix-core image and norms are made once (cs_topk_catalog), like the
        # reference embeds `lib_desc` once before it ranks the scans (evaluation.py:264-283)
        from corsair_amd import backend as B
        self.xcat = B.TopkCatalog(self.x)
        nq = 65536
        self.q = torch.from_numpy(synth.make_descriptors(nq, self.d, seed=1234 + ctx.rank)).to(ctx.dev)
        torch.cuda.synchronize()
        ctx.log("setup done: stress, %d clouds resident, catalog %d x %d in %.1fs" % (self.N_UNIQUE, self.C, self.d,
                                                                                  time.time() - t0))

    def step(self, b):
        from corsair_amd import backend as B

        last = None
        for j in range(self.BATCHES_PER_STEP):
            xyz, off = self.batches[(b * self.BATCHES_PER_STEP + j) % len(self.batches)]
            last = self.pipe.embed_batch(xyz, off)
            self.voxels += last.F.shape[0]
            self.clouds += len(off) - 1
        s = (b * self.TOPK_PER_STEP) % (self.q.shape[0] - self.TOPK_PER_STEP + 1)
        qs = self.q[s:s + self.TOPK_PER_STEP]
        if self.ctx.world == 1:
            idx = B.l2_topk(qs, self.xcat, 10)
        else:
            # catalog sharded over the ranks: all-gather the queries, top-10 per shard, all-gather the candidate
            # lists, merge (the one real exchange of this workload, inside the timed step)
            from corsair_amd import sharding

            idx, _ = sharding.sharded_topk(self.ctx.dist, qs, lambda qq: B.l2_topk(qq, self.xcat, 10, True, squared=True),
                                           self.shard[0], 10, self.ctx.rank, self.ctx.world)
        self.results.append((b, idx[:64].cpu().numpy(), last.desc[:4].cpu().numpy()))
        if b == self.last_step:     # the step's 10 240 top-10 lists and the descriptors of its last forward batch
            self.last_out = {"topk_ids": idx, "desc_last_batch": last.desc}

    def same_results(self, a, b):
        return np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])

    def solo_env(self):
        return None

    def config(self, steps):
        import ctypes

        from corsair_amd import _lib

        st = (ctypes.c_uint64 * 2)()
        _lib.load().cs_l2_topk_stats(st, 0)
        return {"workload": "configs[4]: synthetic stress -- batch-64 sparse ResUNetBN2C forward + embedding on "
                            "15k-pt clouds @ 2 cm voxels, and top-10 of %d-d descriptors against a %d catalog; "
                            "one step = 1024 clouds (16 batches) + 10240 top-10 queries (the clouds' share of "
                            "10^6 x 10^6); a 'query' here = one cloud embedded + its 10 top-10 look-ups"
                            % (self.d, self.C),
                "queries_per_step": self.units_per_step, "catalog": self.C, "desc_dim": self.d,
                "voxels_per_cloud": self.voxels / max(self.clouds, 1),
                "topk_f16_shortlist_queries": int(st[0]), "topk_recomputed_by_f64_path": int(st[1])}

    def extras(self, out):
        pass

    def cpu_baseline(self):
        """Oracle forward + embedding of a 2-cloud batch and oracle top-10 of 32 queries against the
        first 131 072 catalog rows, scaled to the step's mix (1 cloud : 10 look-ups against C rows)."""
        from oracle import native, resunet as oref, sparse as osp

        native.load()
        t0 = time.time()
        grids = [osp.quantize_cloud(pc, self.cfg.voxel_size)[1] for pc in self.cloud_sample]
        coords = osp.sparse_collate(grids)
        feats = np.ones((coords.shape[0], 1), np.float32)
        out, feat8, maps = oref.resunet_forward(self.sd, coords, feats)
        oref.embedding_forward(self.emb, feat8, maps["c8"][:, 0], len(grids))
        t_fwd = (time.time() - t0) / len(grids)
        nq, nx = 32, min(131072, self.C)
        q = self.q[:nq].cpu().numpy()
        x = self.x[:nx].cpu().numpy()
        t1 = time.time()
        d2 = native.dist2_matrix(q, x)
        np.argsort(d2, axis=1, kind="stable")[:, :10]
        t_top = (time.time() - t1) / nq * (self.C / nx)
        per_cloud = t_fwd + 10 * t_top
        return {"value": 1.0 / per_cloud, "unit": "queries/s", "cores": native.num_threads(), "kind": "port",
                "sample": "oracle forward+embedding of a 2-cloud batch (%.2fs per cloud) + exact f64 top-10 of %d "
                          "queries against %d rows scaled to %d rows (%.3fs per look-up); one 'query' = 1 cloud "
                          "+ 10 look-ups" % (t_fwd, nq, nx, self.C, t_top)}


# =====================================================================================================
def roofline_of(fam, solo, args):
    """Roofline object for the dominant kernel family of the timed region.  `achieved` follows SURVEY
    8d's algorithmic units: 30 FLOP per (hypothesis, pair) for the RANSAC inlier count -- whichever
    kernel evaluates it --, 2 pairs Cin Cout for the convolutions, 2 Q C d for the top-k."""
    dom = max(KERNEL_OF, key=lambda k: fam[k]["ms"])
    d = fam[dom]
    peak = PEAK_OF.get(dom, F32_PEAK_TFLOPS)
    n = max(d["launches"], 1)
    achieved = d["flop"] / (max(d["ms"], 1e-9) * 1e-3) / 1e12
    r = {"bound": "mfma", "kernel": KERNEL_OF[dom], "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
         "frac": achieved / peak, "traffic": None, "avg_launch_ms": d["ms"] / n, "launches": d["launches"],
         "flop_per_launch": d["flop"] / n, "concurrent": dom == "ransac_pre",
         "units": {"ransac_pre": "30 FLOP per (hypothesis, pair) (SURVEY 8d), peak = dense f16 MFMA",
                   "ransac_eval": "30 FLOP per (hypothesis, pair) (SURVEY 8d), peak = f32 MFMA",
                   "conv": "2 x pairs x Cin x Cout (SURVEY 8d), peak = f32 MFMA (v_mfma_f32_32x32x2_f32)",
                   "topk": "2 Q C d (SURVEY 8d), peak = dense f16 MFMA",
                   "knn": "2 N0 N1 16 (SURVEY 8d), peak = dense f16 MFMA",
                   "chamfer": "8 N0 N1 (SURVEY 8d), peak = dense f16 MFMA (the ranking executes 32 N0 N1)"}[dom]}
    if dom == "ransac_pre":
        # the matrix pipe executes K f16 multiply-adds per (hypothesis, pair): K = 16 (a_hi . b_hi', round 4 default) or
        # 32 (a_hi . (b_hi + b_lo), CS_RANSAC_PF_K=32)
        pf_k = 32 if os.environ.get("CS_RANSAC_PF_K", "16") == "32" else 16
        ex = 2.0 * pf_k / 30.0
        r["executed_flop_per_pair"] = 2 * pf_k
        r["achieved_executed"] = achieved * ex
        r["frac_executed"] = r["achieved_executed"] / peak
        if solo and solo["launches"]:
            a_solo = solo["flop"] / (solo["ms"] * 1e-3) / 1e12
            r["solo"] = {"achieved": a_solo, "frac": a_solo / peak, "frac_executed": a_solo * ex / peak,
                         "avg_launch_ms": solo["ms"] / solo["launches"], "launches": solo["launches"],
                         "note": "same kernel and inputs with CS_RANSAC_OVERLAP=0 CORSAIR_SPLIT_RANSAC=0 "
                                 "(nothing else on the GPU while it runs), extra untimed pass"}
    if dom == "conv":
        r["bound_note"] = ("the layer is bound by the f32 matrix pipe, not by HBM: the gathered rows are served on chip (L2 / "
                           "Infinity Cache; the PMC `traffic` is ~4.8x the algorithmic bytes with those hits included, DESIGN 7), so "
                           "north_star's '>= 70 % HBM utilisation in the gather' is the wrong yardstick for this kernel -- the gather "
                           "moves 2.6 TB/s = 0.33 of the HBM peak while the MFMA chain sits at the `frac` above")
    if dom == "topk":
        r["achieved_executed"] = achieved * 3.0   # x_hi q_hi + x_lo q_hi + x_hi q_lo
        r["frac_executed"] = r["achieved_executed"] / peak
    # HBM bytes per launch and SQ pipe-busy fractions of the dominant kernel from separate rocprofv3 --pmc
    # runs of this same command (profiles/pmc_<workload>.json, tools/pmc_collect.sh).  They describe the kernels
    # they were collected on: attached only while corsair_amd/csrc is byte-identical to that collection
    pmc = load_pmc(args.workload)
    if pmc is None:
        r["counters"] = "none collected for this workload"
    elif pmc.get("csrc_sha") != csrc_sha():
        r["counters"] = "stale: profiles/pmc_%s.json was collected on other kernel sources (%s, now %s)" % (
            args.workload, pmc.get("csrc_sha"), csrc_sha())
    elif pmc.get("kernel") == r["kernel"]:
        r["traffic"] = pmc.get("hbm_bytes_per_launch")
        for k in ("mfma_busy", "valu_active", "wait_any", "source"):
            if k in pmc:
                r[k if k != "source" else "counters_source"] = pmc[k]
    return r


_CSRC_SHA = None


def csrc_sha():
    """Hash of the kernel sources (same function as tools/pmc_to_json.py)."""
    global _CSRC_SHA
    if _CSRC_SHA is None:
        import hashlib

        h = hashlib.sha256()
        d = os.path.join(ROOT, "corsair_amd", "csrc")
        for f in sorted(os.listdir(d)):
            if f.endswith((".hip", ".h")):
                with open(os.path.join(d, f), "rb") as fh:
                    h.update(fh.read())
        _CSRC_SHA = h.hexdigest()[:16]
    return _CSRC_SHA


def load_pmc(workload):
    tpath = os.path.join(ROOT, "profiles", "pmc_%s.json" % workload)
    if not os.path.exists(tpath):
        return None
    with open(tpath) as f:
        return json.load(f)


def roofline_by_kernel(fam, args):
    """Per kernel family of the timed region: achieved TFLOP/s in SURVEY 8d units (this run's event time) and --
    where the committed PMC pass matches the kernel sources -- HBM GB/s = PMC bytes per library call x this run's
    calls / this run's event time, with the fraction of the 8 TB/s HBM peak, and the matrix-pipe busy share."""
    pmc = load_pmc(args.workload)
    fresh = pmc is not None and pmc.get("csrc_sha") == csrc_sha()
    out = {}
    for name in FAMILIES:
        d = fam.get(name)
        if not d or d["launches"] == 0 or d["ms"] <= 0:
            continue
        e = {"ms": round(d["ms"], 3), "calls": d["launches"]}
        if d["flop"] > 0:
            tf = d["flop"] / (d["ms"] * 1e-3) / 1e12
            peak = PEAK_OF.get(name, F32_PEAK_TFLOPS)
            e.update({"tflops": round(tf, 2), "peak_tflops": peak, "frac_of_matrix_peak": round(tf / peak, 4)})
        pf = pmc.get("families", {}).get(name) if fresh else None
        if pf:
            gbs = pf["hbm_bytes_per_call"] * d["launches"] / (d["ms"] * 1e-3) / 1e9
            e.update({"hbm_gb_s": round(gbs, 1), "frac_of_hbm_peak": round(gbs / 8000.0, 4),
                      "hbm_mb_per_call": round(pf["hbm_bytes_per_call"] / 1e6, 2),
                      "mfma_busy": round(pf["mfma_busy"], 3), "valu_active": round(pf["valu_active"], 3)})
        out[name] = e
    if not fresh:
        out["counters"] = "none" if pmc is None else "stale (profiles/pmc_%s.json predates the kernel sources)" % args.workload
    return out


class Runner:
    """Runs steps [first, last) of a workload with `depth` batches in flight.  Worker threads are PERSISTENT (one
    single-thread executor each): the library caches scratch per host thread and the helper thread / streams of a
    worker are created on its first step, so a worker that is started for the timed pass only would pay hipMalloc
    and thread start-up inside the timed region."""

    # Worker threads and their streams are shared by every Runner of the process (headline and legs).  The library keeps
    # per-thread side streams (RANSAC front halves, kernel-map levels) for the life of a thread and HIP maps all streams of
    # the process onto a handful of hardware queues: a leg that started fresh threads doubled the live streams, its workers'
    # streams then shared queues, and its batches-in-flight pass fell BELOW its sequential pass (profiles/r5x_*: table leg
    # 757 - 770 in flight against 820 sequential).
    _workers = {}
    _streams = []

    def __init__(self, ctx, wl, depth):
        import torch

        self.ctx, self.wl, self.depth = ctx, wl, depth
        self.group = max(1, int(getattr(ctx.args, "embed_group", 1)))
        if not ctx.dry:
            while len(Runner._streams) < max(depth, IN_FLIGHT[0], 3):
                Runner._streams.append(torch.cuda.Stream(device=ctx.dev))
        self.streams = Runner._streams
        self.workers = Runner._workers

    def worker_of(self, w):
        from concurrent.futures import ThreadPoolExecutor

        if w not in self.workers:
            self.workers[w] = ThreadPoolExecutor(max_workers=1, thread_name_prefix="bench-worker%d" % w)
        return self.workers[w]

    def run_steps(self, first, last, depth=None):
        import torch

        depth = self.depth if depth is None else depth
        wl, ctx, streams = self.wl, self.ctx, self.streams
        # A workload with step_group and --embed-group N > 1: the query batches of N consecutive steps go through ONE forward
        # of the network (groups formed from `first`: never across the timed region's edge); retrieval and registration stay
        # per step.  One batch at a time: a group is the work item.  Several in flight: the STEP stays the work item (a group
        # would be too coarse at the ragged end of a short run); the worker that first needs a group runs its forward on its own
        # stream, the others wait for that stream's event and then register their steps -- one forward per group, three
        # registrations in flight.
        n_grp = self.group if hasattr(wl, "step_group") else 1
        if depth == 1:
            for b in range(first, last, n_grp):
                item = list(range(b, min(b + n_grp, last)))
                if len(item) > 1:
                    wl.step_group(item)
                else:
                    wl.step(item[0])
            return

        import threading
        from concurrent.futures import Future

        lock = threading.Lock()
        shared = {}      # group index -> Future of ({step: EmbeddedSet}, event recorded behind the forward)

        def embedded(b):
            g = (b - first) // n_grp
            with lock:
                fut = shared.get(g)
                mine = fut is None
                if mine:
                    fut = shared[g] = Future()
            if mine:
                try:
                    steps = list(range(first + g * n_grp, min(first + (g + 1) * n_grp, last)))
                    sets = wl.embed_steps(steps)
                    ev = torch.cuda.Event()
                    ev.record()                       # on this worker's stream, behind the forward
                    fut.set_result((sets, ev))
                except BaseException as e:            # noqa: BLE001 -- the waiting workers must not hang
                    fut.set_exception(e)
                    raise
            sets, ev = fut.result()
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            qs = sets[b]
            for t in (qs.F, qs.origin, qs.desc):     # allocated on the embedding worker's stream, used on this one
                t.record_stream(cur)
            return qs

        def work(w):
            if ctx.dry:                                  # no device: the host-thread plumbing alone
                for b in range(first + w, last, depth):
                    wl.step(b)
                return
            torch.cuda.set_device(ctx.dev_index)
            with torch.cuda.stream(streams[w]):
                for b in range(first + w, last, depth):
                    if n_grp > 1:
                        wl.register_step(b, embedded(b))
                    else:
                        wl.step(b)
                streams[w].synchronize()

        futures = [self.worker_of(w).submit(work, w) for w in range(depth)]
        for f in futures:
            f.result()              # surfaces worker failures in the main thread

    def close(self):
        """(the shared workers live until the process ends: see above)"""


def bracketed(ctx, runner, first, last, depth=None):
    """Steps [first, last) bracketed by barrier + torch.cuda.synchronize() on both sides: the bracket of every timed pass
    (timed_region, piped_pass, in_flight_region).  Everything allocated so far (the catalog, K + W batches of query clouds,
    the network) is long-lived: moved to the permanent generation so that a full collection of Python's cycle collector
    inside the region does not walk it (measured: 10 - 50 ms pauses in some steps of a 20-step run, 1 360 vs 1 485 q/s;
    BENCH_GC=1 keeps the default).  Thawed again right after the region: a leg's workload must be collectable
    before the next leg starts.  Returns (barrier-to-barrier seconds, this rank's own seconds)."""
    frozen = os.environ.get("BENCH_GC", "freeze") == "freeze"
    if frozen:
        gc.collect()
        gc.freeze()
    try:
        ctx.barrier()
        t_start = time.time()
        runner.run_steps(first, last, depth=depth)
        ctx.sync()
        own_elapsed = time.time() - t_start
        ctx.barrier()
        elapsed = time.time() - t_start
    finally:
        if frozen:
            gc.unfreeze()
    return elapsed, own_elapsed


def timed_region(ctx, wl, runner, warmup, steps):
    """The contract's measurement: W untimed warmup steps, then EXACTLY K steps bracketed by barrier +
    torch.cuda.synchronize() on both sides, the library's HIP-event profile (events on the launch streams) switched on
    for exactly those steps.  Returns (barrier-to-barrier seconds, this rank's own seconds, per-family profile)."""
    import torch

    from corsair_amd import _lib

    runner.run_steps(0, warmup)
    ctx.log("warmup done")
    wl.results.clear()
    if not ctx.dry:
        _lib.prof_enable(True)
        _lib.prof_reset()
    elapsed, own_elapsed = bracketed(ctx, runner, warmup, warmup + steps)
    fam = {}
    if not ctx.dry:
        _lib.prof_enable(False)
    ctx.log("timed region: %d steps in %.3fs" % (steps, elapsed))
    for name in FAMILIES:
        ms, n, units = (0.0, 0, 0.0) if ctx.dry else _lib.prof_get(name)
        fam[name] = {"ms": ms, "launches": n, "flop": units}
    return elapsed, own_elapsed, fam


def piped_pass(ctx, wl, runner, warmup, steps):
    """The same K steps again with several batches in flight (IN_FLIGHT host threads, one HIP stream each), bracketed like the
    timed region (barrier + synchronize on both sides), results compared with the pass before.  Returns (seconds,
    identical).  The library's event profile stays off: launches of different batches share the GPU here."""
    seq_results = {r[0]: r for r in wl.results}
    runner.run_steps(0, min(IN_FLIGHT[0], warmup + steps), depth=IN_FLIGHT[0])   # untimed: every worker's first step (cold scratch)
    wl.results.clear()
    piped_elapsed, _ = bracketed(ctx, runner, warmup, warmup + steps, depth=IN_FLIGHT[0])
    same = len(wl.results) == len(seq_results) and all(wl.same_results(r, seq_results[r[0]]) for r in wl.results)
    wl.results[:] = [seq_results[b] for b in sorted(seq_results)]
    return piped_elapsed, same


def in_flight_warmup_steps(warmup, steps, depth, group):
    """Untimed steps [0, n) in front of in_flight_region: the W warmup steps, and never fewer than one step per worker
    (no worker meets its cold scratch and streams inside the region) or one whole embed group (the first forward of a
    group as large as the timed ones runs before the region); at most W + K."""
    return min(warmup + steps, max(warmup, depth, group))


def in_flight_region(ctx, wl, runner, warmup, steps):
    """A run without --full whose `value` comes from the batches-in-flight pass times that pass alone: the untimed
    in_flight_warmup_steps with IN_FLIGHT batches in flight, then EXACTLY K steps in the bracket of every timed pass.
    Unlike --full, nothing compares this pass's results with the sequential pass (`batches_in_flight.identical_results`
    of a --full run does).  Returns (barrier-to-barrier seconds, this rank's own seconds)."""
    depth = IN_FLIGHT[0]
    group = runner.group if hasattr(wl, "step_group") else 1
    runner.run_steps(0, in_flight_warmup_steps(warmup, steps, depth, group), depth=depth)
    ctx.log("warmup done")
    wl.results.clear()
    elapsed, own_elapsed = bracketed(ctx, runner, warmup, warmup + steps, depth=depth)
    ctx.log("timed region: %d steps in %.3fs, %d batches in flight" % (steps, elapsed, depth))
    wl.results.sort(key=lambda r: r[0])       # the workers finish their steps in any order
    return elapsed, own_elapsed


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(wl, out_dir):
    """--dump-outputs: the arrays the last timed step returned, one DIR/<name>.npy each -- floating point as float32 /
    float64, ids, counts and flags as float64 (exact below 2^53).  An array that would take the files past 64 MB in all
    is cut to a fixed sample of its rows (seed 0, rows in order)."""
    if wl.last_out is None:
        raise RuntimeError("--dump-outputs: the last timed step recorded no outputs")
    arrays = {}
    for name, v in wl.last_out.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        arrays[name] = a.astype(np.float32 if a.dtype in (np.float16, np.float32) else np.float64)
    share = DUMP_LIMIT_BYTES // max(len(arrays), 1)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if a.nbytes > share and a.ndim > 0:
            keep = max(1, share // max(a.nbytes // max(len(a), 1), 1))
            a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def overlap_probe_allowed(depth, steps, disabled, world, wl):
    """The extra `batches_in_flight` pass runs three batches on three host threads.  With a collective inside the step
    on several ranks the worker threads of a rank would issue their all-gathers in an order of their own and the
    ranks' collectives would no longer pair up (the crash fixed in 86a7de4): never in that case.  Strong-scaling steps
    are whole evaluations, not independent batches: never there either."""
    if depth != 1 or steps < 2 or disabled:
        return False
    if getattr(wl, "scaling", "weak") == "strong":
        return False
    return not (world > 1 and getattr(wl, "collective_in_step", False))


LEG_STEPS, LEG_WARMUP = 8, 2
IN_FLIGHT = [3]     # batches in flight of the pass that gives `value` (--in-flight)


def auto_in_flight(steps):
    """Depth of the batches-in-flight pass.  Steps are dealt to the workers round-robin, so K steps at depth d take
    ceil(K / d) rounds: the depth in 3..6 with the fullest rounds, the larger one on ties.  With eight hardware queues the
    chair rate still rises from three to five / six batches in flight (1 870 - 1 947 -> 1 987 - 2 016 queries/s) and stress from three to
    four (9 595 - 9 774 -> 9 950 - 9 994 clouds/s); table is flat (profiles/r5s_in_flight_depth_sweep.txt)."""
    best, best_eff = 3, 0.0
    for d in (3, 4, 5, 6):
        eff = steps / float(d * -(-steps // d))
        if eff >= best_eff - 1e-12:
            best, best_eff = d, eff
    return best


def extra_workload_leg(ctx, args, name):
    """One short leg of another BASELINE.json config inside the default run (configs[2] and configs[4]
    under the driver's clock): the same timed_region as the headline (2 warmup + 8 timed steps, sequential), on its own
    workload object, reported under `workloads[name]` with the same arithmetic (value = units / elapsed)."""
    import copy

    import torch

    leg_args = argparse.Namespace(**vars(args))
    leg_args.workload, leg_args.steps, leg_args.warmup, leg_args.catalog, leg_args.pipeline = name, LEG_STEPS, LEG_WARMUP, 0, 1
    lctx = copy.copy(ctx)
    lctx.args = leg_args
    t0 = time.time()
    if name == "converging":
        leg_args.workload = "chair"
        wl = RegistrationWorkload(lctx, "chair", converging=True)
    else:
        wl = StressWorkload(lctx) if name == "stress" else RegistrationWorkload(lctx, name)
    wl.setup()
    runner = Runner(lctx, wl, 1)
    elapsed, _, fam = timed_region(lctx, wl, runner, LEG_WARMUP, LEG_STEPS)
    cfg = wl.config(LEG_STEPS)
    units = LEG_STEPS * wl.units_per_step
    # the same second pass as the headline: the K steps again with several batches in flight, results compared
    saved_depth = IN_FLIGHT[0]
    if args.in_flight <= 0:
        IN_FLIGHT[0] = auto_in_flight(LEG_STEPS)
    try:
        piped_elapsed, same = piped_pass(lctx, wl, runner, LEG_WARMUP, LEG_STEPS)
    finally:
        leg_depth, IN_FLIGHT[0] = IN_FLIGHT[0], saved_depth
    runner.close()
    piped = bool(same)        # the headline pass is fixed a priori (see main): three in flight whenever the results are identical
    head = piped_elapsed if piped else elapsed
    leg = {"value": units / head, "unit": "queries/s", "steps": LEG_STEPS, "warmup": LEG_WARMUP,
           "ms_per_step": head / LEG_STEPS * 1e3, "value_pass": ("%d batches in flight" % leg_depth) if piped else "sequential",
           "sequential": {"value": units / elapsed, "ms_per_step": elapsed / LEG_STEPS * 1e3},
           "batches_in_flight": {"value": units / piped_elapsed, "ms_per_step": piped_elapsed / LEG_STEPS * 1e3,
                                 "identical_results": bool(same), "depth": leg_depth},
           "units_per_step": wl.units_per_step,
           "config": cfg, "roofline": roofline_of(fam, None, leg_args),
           "kernel_ms": {k: round(v["ms"], 3) for k, v in fam.items()}}
    leg["roofline"]["pass"] = "sequential"
    if hasattr(wl, "step_group"):
        leg["config"]["embed_batches_per_forward"] = max(1, leg_args.embed_group)   # sequential pass (see the headline's note)
    if name == "stress":
        leg["kernel_tflops"] = {k: round(fam[k]["flop"] / max(fam[k]["ms"], 1e-9) / 1e9, 2) for k in ("conv", "topk")}
        leg["est_full_job_s"] = 100000.0 / leg["value"]   # 100 k clouds + the whole 10^6 x 10^6 top-10
    del wl, runner
    gc.collect()              # the leg's workload (catalog, network, worker closures) goes before the next leg allocates
    torch.cuda.empty_cache()
    leg["leg_wall_s"] = round(time.time() - t0, 2)
    return leg


def leg_summary(leg):
    """What `config.legs.<name>` carries of a leg: its value (unit named), the pass it comes from, both passes, the dominant
    kernel's roofline fraction."""
    r = leg["roofline"]
    out = {"value": round(leg["value"], 1), "unit": "clouds/s (1 cloud + its 10 top-10 look-ups)" if "est_full_job_s" in leg
           else "queries/s", "ms_per_step": round(leg["ms_per_step"], 3), "steps": leg["steps"], "value_pass": leg["value_pass"],
           "sequential_value": round(leg["sequential"]["value"], 1),
           "identical_results": leg["batches_in_flight"]["identical_results"],
           "dominant_kernel": r["kernel"], "roofline_frac": round(r["frac"], 4), "roofline_peak": "%s %s" % (r["peak"], r["unit"]),
           "workload": leg["config"]["workload"].split(":")[0]}
    if "est_full_job_s" in leg:
        out["est_full_job_s"] = round(leg["est_full_job_s"], 2)
        out["kernel_tflops"] = leg["kernel_tflops"]
    for k in ("top1_hit_rate", "rre_mean_deg", "rre_5", "rre_15", "rte_010", "ransac_mean_iters", "ransac_early_exit_share"):
        if k in leg["config"]:
            out[k] = leg["config"][k]
    return out


class DryWorkload:
    """`--workload dry`: no kernels and no GPU.  A step is a few microseconds of host arithmetic; the setup runs the
    sharding collectives of the real workloads on tiny stand-in sets.  What it exercises is everything AROUND the path at
    N ranks -- the child torchrun, rank layout, the gloo control plane, barriers, max-over-ranks timing, three host threads
    per rank, exactly one JSON line on rank 0's stdout (tests/test_bench_launch_cpu.py, 8 CPU ranks).  Never a measurement:
    the line says so."""

    def __init__(self, ctx):
        self.ctx, self.results, self.units_per_step = ctx, [], BATCH
        self.last_step, self.last_out = ctx.args.warmup + ctx.args.steps - 1, None

    def setup(self):
        import torch

        from corsair_amd import sharding
        from corsair_amd.harness import EmbeddedSet

        ctx, C = self.ctx, 11
        mine = sharding.shard_ids(C, ctx.rank, ctx.world)
        vox = sharding.all_gather_counts(ctx.dist, mine, [100 + 7 * c for c in mine], C, ctx.world)
        shards = sharding.balanced_shards(vox, ctx.world)

        def item(c):
            return torch.full((3 + c % 4, 16), float(c)), torch.full((3 + c % 4, 3), -float(c)), torch.full((1, 256), float(c))

        parts = [item(c) for c in shards[ctx.rank]]
        off = np.concatenate([[0], np.cumsum([len(p_[0]) for p_ in parts])]).astype(int).tolist()
        local = EmbeddedSet(torch.cat([p_[0] for p_ in parts]) if parts else torch.zeros((0, 16)),
                            torch.cat([p_[1] for p_ in parts]) if parts else torch.zeros((0, 3)), off,
                            torch.cat([p_[2] for p_ in parts]) if parts else torch.zeros((0, 256)))
        self.catalog = sharding.gather_catalog(ctx.dist, local, C, ctx.world, shards)
        assert [float(v) for v in self.catalog.desc[:, 0]] == [float(c) for c in range(C)]

    def step(self, b):
        v = float(np.sin(b + self.ctx.rank))
        self.results.append((b, v))
        if b == self.last_step:
            self.last_out = {"step_value": np.float64(v)}

    def same_results(self, a, b):
        return a == b

    def solo_env(self):
        return None

    def config(self, steps):
        return {"workload": "DRY RUN -- no kernels, no GPU: launcher / collectives / output plumbing only; not a measurement",
                "catalog": len(self.catalog)}

    def extras(self, out):
        pass


def main():
    args = parse()
    # HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (runtime default 4).  A step with three batches in
    # flight keeps ~12 streams busy (three workers x (caller + RANSAC side streams + kernel-map streams)); with 8 queues fewer
    # of them serialise behind each other: chair + 4.5 %, table + 5.7 %, stress +- 0 on alternated runs of one box
    # (profiles/r5q_hw_queues_ab.txt; round 4 measured + 1 - 5 % and a cliff at 16 / 32, which is why it is 8 and not more).
    # Must be in the environment before the first HIP call; an explicit setting of the caller wins.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    IN_FLIGHT[0] = max(2, int(args.in_flight)) if args.in_flight > 0 else auto_in_flight(args.steps)
    maybe_self_launch(args)
    # The contract: rank 0 prints ONE JSON line on stdout.  Libraries write there too (torch's gloo backend announces
    # "[Gloo] Rank 0 is connected to ..." on stdout when the control-plane group comes up): from here on file descriptor 1
    # is stderr, and the result line goes out through a saved copy of the real stdout.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    import torch

    from corsair_amd import _lib

    ctx = Ctx(args)
    if args.scaling == "strong":
        if args.workload == "stress":
            sys.stderr.write("[bench] --scaling strong is the chair / table evaluation; the stress workload is weak-scaled\n")
            sys.exit(2)
        wl = StrongEvalWorkload(ctx, args.workload)
    elif ctx.dry:
        wl = DryWorkload(ctx)
    else:
        wl = StressWorkload(ctx) if args.workload == "stress" else RegistrationWorkload(ctx, args.workload)
    wl.setup()

    # Query batches are independent: `--pipeline D` keeps D of them in flight, each driven by its own
    # host thread on its own HIP stream, so the host work of one batch (index plumbing, the per-chunk
    # RANSAC control loop) overlaps the kernels of another.  D = 1 is the plain sequential loop.
    depth = max(1, min(args.pipeline, args.steps))
    if depth > 1 and ctx.world > 1 and getattr(wl, "collective_in_step", False):
        sys.stderr.write("[bench] --pipeline %d with %d ranks: this workload's step contains a collective, batches in flight "
                         "would interleave the ranks' collectives; refusing\n" % (depth, ctx.world))
        sys.exit(2)
    runner = Runner(ctx, wl, depth)
    run_steps = runner.run_steps
    # Without --full the run times only the pass that gives `value` (the a-priori choice made below): the K steps with
    # several batches in flight where that pass is allowed, else the sequential timed region.  --full times both passes and
    # compares their results, and adds the probes, legs and baselines after them.
    lean_piped = (not args.full and not args.sequential_value
                  and overlap_probe_allowed(depth, args.steps, args.no_overlap_probe, ctx.world, wl))
    fam = solo = overlap = None
    if lean_piped:
        elapsed, own_elapsed = in_flight_region(ctx, wl, runner, args.warmup, args.steps)
    else:
        elapsed, own_elapsed, fam = timed_region(ctx, wl, runner, args.warmup, args.steps)
    if args.full:
        # In the timed region the prefilter launches of a step overlap other work (the vanilla and the
        # symmetric RANSAC calls run on two host threads, the small kernels of a round run under the next
        # prefilter), so their event-bracketed durations include the share of the GPU they did not have.
        # A short extra pass with both overlaps switched off gives the kernel's stand-alone rate (same inputs,
        # same launches merged back into one call); reported as roofline.solo, not used for `value`.
        if ctx.world == 1 and not args.no_solo_probe and args.steps >= 1 and wl.solo_env():
            env = wl.solo_env()
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                keep = list(wl.results)
                _lib.prof_reset()
                _lib.prof_enable(True)
                run_steps(args.warmup, args.warmup + min(2, args.steps), depth=1)
                torch.cuda.synchronize()
                _lib.prof_enable(False)
                ms, n, units = _lib.prof_get("ransac_pre")
                solo = {"ms": ms, "launches": n, "flop": units}
                wl.results[:] = keep
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            ctx.log("stand-alone prefilter pass done")
        # Throughput mode, reported next to the contract number (never instead of it): the same K batches
        # again with three of them in flight.  Kernels of the two streams share the GPU, so per-launch event
        # times are not a roofline measurement there; profiling stays off.  The results must come out
        # identical to the sequential pass.
        # (not with a collective inside the step on several ranks: the worker threads of a rank would issue their
        # all-gathers in an order of their own and the ranks' collectives would no longer pair up)
        if overlap_probe_allowed(depth, args.steps, args.no_overlap_probe, ctx.world, wl):
            overlap = piped_pass(ctx, wl, runner, args.warmup, args.steps)
            ctx.log("%d batches in flight: %d steps in %.3fs, identical results: %s" % (IN_FLIGHT[0], args.steps, overlap[0], overlap[1]))
    # contract: the MAX over ranks of the barrier-to-barrier time; per-rank own times show the balance
    elapsed, ov = ctx.reduce_max([elapsed, overlap[0] if overlap else 0.0])
    if overlap:
        overlap = (ov, overlap[1])
    own = ctx.gather_floats([own_elapsed])[:, 0]

    cfg = wl.config(args.steps)   # every rank (accuracy bookkeeping of its own queries)
    if ctx.rank == 0:
        dumped = dump_outputs(wl, args.dump_outputs) if args.dump_outputs else None
        strong = getattr(wl, "scaling", "weak") == "strong"
        total_units = args.steps * wl.units_per_step * (1 if strong else ctx.world)
        # `value`: the K steps with three batches in flight (three host threads x three HIP streams) WHENEVER that pass ran
        # and its results are identical to the sequential pass -- VERDICT r3 #5: the embed of step i+1 under the RANSAC of
        # step i is real throughput.  The choice is made a priori, not per run by which pass came out faster (the
        # faster of two noisy measurements biases the headline); `--sequential-value` / `--no-overlap-probe` select the
        # sequential pass.  Without --full only the pass that gives `value` runs (in_flight_region or timed_region); with it
        # `sequential` carries the one-batch-at-a-time figures, and `roofline` is measured over THAT pass (in the pipelined
        # one a launch's event time includes its neighbours).
        piped = lean_piped or (overlap is not None and bool(overlap[1]) and not args.sequential_value)
        head_elapsed = overlap[0] if overlap is not None and piped else elapsed
        cfg.update({"parallelism": "dp%d" % ctx.world, "batches_in_flight": IN_FLIGHT[0] if piped else depth,
                    "value_pass": ("%d batches in flight" % IN_FLIGHT[0]) if piped else "sequential",
                    "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")})
        if hasattr(wl, "step_group"):
            cfg["embed_batches_per_forward"] = max(1, args.embed_group)   # both passes
        out = {
            "metric": "end-to-end queries/sec (embed+retrieve+register), Scan2CAD %s"
                      % ("chair" if args.workload == "stress" else args.workload),
            "value": total_units / head_elapsed,
            "unit": "queries/s",
            "n_gpus": ctx.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": head_elapsed / args.steps * 1e3,
            "value_pass": ("%d batches in flight" % IN_FLIGHT[0]) if piped else "sequential",
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": DTYPE_LABEL[args.workload if args.workload in ("stress", "dry") else "registration"],
            "data": "none (dry run)" if ctx.dry else "synthetic",
            "config": cfg,
        }
        if args.full:
            out.update({"roofline": None if ctx.dry else roofline_of(fam, solo, args),
                        "roofline_by_kernel": None if ctx.dry else roofline_by_kernel(fam, args),
                        "kernel_ms": {k: round(v["ms"], 3) for k, v in fam.items()}})
        if ctx.dry:
            out["metric"] = "DRY RUN (no kernels): steps/s of an empty step"
        if args.workload == "stress":
            out["metric"] = "stress queries/sec (batch-64 forward + top-10 share), configs[4]"
            if args.full:
                out["kernel_tflops"] = {k: round(fam[k]["flop"] / max(fam[k]["ms"], 1e-9) / 1e9, 2)
                                        for k in ("conv", "topk")}
            out["est_full_job_s"] = 100000.0 / out["value"]  # 100k clouds + 10^6 x 10^6 top-10 (value = all ranks)
        if ctx.world > 1:
            out["dist"] = {"backend": "rccl" if ctx.backend == "nccl" else ctx.backend,
                           "devices_visible": ctx.n_devices,
                           "rank_elapsed_s": [round(float(v), 4) for v in own],
                           "rank_time_max_over_min": float(own.max() / max(own.min(), 1e-9))}
        wl.extras(out)
        if dumped is not None:
            out["outputs_dumped"] = dumped
        if args.full:
            out["sequential"] = {"value": total_units / elapsed, "unit": "queries/s", "ms_per_step": elapsed / args.steps * 1e3,
                                 "note": "the same K steps one batch at a time (the pass `roofline`, `roofline_by_kernel` and "
                                         "`kernel_ms` are measured over: their launches share the GPU only with their own step)"
                                         + ("; %d consecutive steps' query batches share one forward of the network, retrieval and "
                                            "registration per step" % args.embed_group
                                            if hasattr(wl, "step_group") and args.embed_group > 1 and depth == 1 else "")}
        if out.get("roofline"):
            out["roofline"]["pass"] = "sequential"
        if overlap:
            out["batches_in_flight"] = {
                "depth": IN_FLIGHT[0], "value": total_units / overlap[0], "unit": "queries/s",
                "ms_per_step": overlap[0] / args.steps * 1e3, "identical_results": bool(overlap[1]),
                "is_headline": bool(piped),
                "note": "the same K batches with `depth` host threads, one HIP stream each (the library's scratch cache is per "
                        "thread and stream-ordered); results compared with the sequential pass"}
        if args.full and ctx.world == 1 and args.workload == "chair" and not strong and not args.no_extra_workloads:
            # configs[2] and configs[4] under the same clock as the headline (short legs, same measurement).  BEFORE the
            # CPU baseline: after it the table leg measured 429 instead of 568 queries/s on the same box (the oracle's
            # OpenMP / BLAS worker threads keep the host cores busy for a while after their last parallel region)
            out["workloads"] = {name: extra_workload_leg(ctx, args, name) for name in ("table", "stress", "converging")}
            # the driver's record keeps `config` whole and of everything else only the key names: the legs'
            # figures that matter go there too
            cfg["legs"] = {name: leg_summary(leg) for name, leg in out["workloads"].items()}
        if args.full and ctx.world == 1 and not args.no_cpu_baseline and hasattr(wl, "cpu_baseline"):
            out["cpu_baseline"] = wl.cpu_baseline()
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if ctx.dist is not None:
        ctx.dist.barrier()
        ctx.dist.destroy_process_group()


if __name__ == "__main__":
    main()

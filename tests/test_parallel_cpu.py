"""world_size-2 gloo tests of the data-parallel path (CPU): sharding, result gathering, gradient all-reduce."""

import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfol_vqa_amd import parallel  # noqa: E402
from dfol_vqa_amd.fol_types import QuestionType  # noqa: E402


def test_shard_bounds_are_contiguous_and_balanced():
    rng = np.random.RandomState(0)
    for world in (1, 2, 4, 8):
        costs = rng.randint(1, 100, 57) ** 2
        b = parallel.shard_bounds(costs, world)
        assert b[0][0] == 0 and b[-1][1] == len(costs)
        assert all(b[i][1] == b[i + 1][0] for i in range(world - 1))
        loads = [costs[s:e].sum() for s, e in b]
        assert max(loads) <= costs.sum() / world + costs.max()
    assert parallel.shard_bounds([1, 1, 1, 1], 2) == [(0, 2), (2, 4)]
    assert parallel.shard_bounds([], 2) == [(0, 0), (0, 0)]
    qs = [{"scene": {"n": n}} for n in (10, 10, 10, 10)]
    assert parallel.shard_questions(qs, 1, 2) == qs[2:]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # ---- result gathering keeps question order -------------------------------------------------
        lp = torch.tensor([-0.1 * (rank + 1), -0.2 * (rank + 1), -0.3]) if rank == 0 else torch.tensor([-1.0, -2.0])
        res = {"answer": [["yes"]] * len(lp), "log_probability": lp, "options": ["no", "yes"], "variable_set": None,
               "type": QuestionType.BINARY, "cumulative_loss": 0, "variable_sets_num": len(lp), "answer_log_probability": [[float(x)] for x in lp]}
        g = parallel.gather_results(res)
        assert g["log_probability"].tolist() == [-0.1, -0.2, -0.3, -1.0, -2.0] or np.allclose(g["log_probability"].numpy(), [-0.1, -0.2, -0.3, -1.0, -2.0])
        assert len(g["answer"]) == 5 and g["variable_sets_num"] == 5

        # ---- one flat-bucket all-reduce reproduces the single-process gradient ----------------------
        torch.manual_seed(0)
        model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Sigmoid(), torch.nn.Linear(5, 1))
        model[0].bias.requires_grad_(False)
        x = torch.randn(8, 6)
        y = (torch.rand(8, 1) > 0.5).float()
        B = x.shape[0]
        s, e = parallel.shard_bounds([1.0] * B, world)[rank]
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model(x[s:e]), y[s:e], reduction="sum") / B   # sum / B_global
        loss.backward()
        nbytes = parallel.allreduce_gradients(model.parameters())
        grads = [p.grad.clone() for p in model.parameters() if p.requires_grad]
        if rank == 0:
            ref = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Sigmoid(), torch.nn.Linear(5, 1))
            ref.load_state_dict(model.state_dict())
            ref[0].bias.requires_grad_(False)
            torch.nn.functional.binary_cross_entropy_with_logits(ref(x), y, reduction="sum").div(B).backward()
            for gmine, p in zip(grads, [p for p in ref.parameters() if p.requires_grad]):
                assert torch.allclose(gmine, p.grad, atol=1e-6)
            assert nbytes == 4 * sum(p.numel() for p in ref.parameters() if p.requires_grad)
        # every rank ends with identical gradients
        flat = torch.cat([g_.reshape(-1) for g_ in grads])
        both = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1])

        # ---- replicas that start different are made equal by ONE broadcast (params and buffers) ------
        torch.manual_seed(100 + rank)
        m2 = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 1))
        m2[1].running_mean.add_(rank + 1.0)
        before = parallel.parameters_digest(m2)
        nb = parallel.broadcast_parameters(m2, src=0)
        assert nb == 4 * (sum(p.numel() for p in m2.parameters()) + sum(b.numel() for b in m2.buffers() if b.numel()))
        dg = parallel.parameters_digest(m2)
        both = [torch.zeros_like(dg) for _ in range(world)]
        dist.all_gather(both, dg)
        assert torch.equal(both[0], both[1])
        assert rank == 0 or not torch.equal(before, dg)
        rm = [torch.zeros_like(m2[1].running_mean) for _ in range(world)]
        dist.all_gather(rm, m2[1].running_mean)
        assert torch.equal(rm[0], rm[1])

        # ---- persistent bucket + the step's L1 term: 2-rank step == single-process step ----------------
        from dfol_vqa_amd import training
        torch.manual_seed(7)
        net = torch.nn.Linear(6, 1)
        xs, ys = torch.randn(8, 6), (torch.rand(8) > 0.5)
        lam = 0.3

        class _PB(object):
            def __init__(self, answers):
                self._answers = answers

            def batch_size(self):
                return len(self._answers)

        class _Model(torch.nn.Module):
            def __init__(self, lin):
                super(_Model, self).__init__()
                self.lin = lin

            def forward(self, data, is_training):
                lp = torch.nn.functional.logsigmoid(self.lin(data[0].x)).reshape(-1)
                return {"log_probability": lp, "type": QuestionType.BINARY, "options": ["no", "yes"]}

        def step(lin, lo, hi, group, world_b):
            model = _Model(lin)
            pb = _PB(["yes" if y else "no" for y in ys[lo:hi]])
            pb.x = xs[lo:hi]
            params = list(model.parameters())
            opt = torch.optim.SGD(params, lr=0.1)
            bucket = parallel.GradBucket(params)
            training.train_batch(model, opt, [pb], clip_norm=1e9, global_batch_size=world_b, group=group, l1_lambda=lam, bucket=bucket)
            assert all(p.grad.data_ptr() >= bucket.flat.data_ptr() for p in params)     # the views survived the step
            return torch.cat([p.detach().reshape(-1) for p in params])

        import copy
        s2, e2 = parallel.shard_bounds([1.0] * 8, world)[rank]
        sharded = step(copy.deepcopy(net), s2, e2, dist.group.WORLD, 8)
        single = step(copy.deepcopy(net), 0, 8, None, None)
        assert torch.allclose(sharded, single, atol=1e-6), (sharded, single)

        # the same through the overlapped bucket (three ranges, all-reduced from post-accumulate-grad hooks during the backward): equal to
        # the single-process step; and with rank 1 skipping the middle layer (its range gets no gradient there, and the ranks' graphs
        # finish their ranges in different orders) the collectives still pair up and the replicas stay equal
        class _Deep(torch.nn.Module):
            def __init__(self, skip_mid=False):
                super(_Deep, self).__init__()
                torch.manual_seed(5)
                self.l1, self.l2, self.l3 = torch.nn.Linear(6, 16), torch.nn.Linear(16, 16), torch.nn.Linear(16, 1)
                self.skip_mid = skip_mid

            def forward(self, data, is_training):
                h = torch.relu(self.l1(data[0].x))
                if not self.skip_mid:
                    h = torch.relu(self.l2(h))
                return {"log_probability": torch.nn.functional.logsigmoid(self.l3(h)).reshape(-1), "type": QuestionType.BINARY,
                        "options": ["no", "yes"]}

        def deep_step(lo, hi, group, world_b, overlap, skip_mid=False):
            model = _Deep(skip_mid)
            pb = _PB(["yes" if y else "no" for y in ys[lo:hi]])
            pb.x = xs[lo:hi]
            params = list(model.parameters())
            opt = torch.optim.SGD(params, lr=0.1)
            bucket = parallel.GradBucket(params)
            if overlap:
                bucket.enable_overlap(group, segments=3)
                assert len(bucket._segments) == 3
            training.train_batch(model, opt, [pb], clip_norm=1e9, global_batch_size=world_b, group=group, bucket=bucket)
            training.train_batch(model, opt, [pb], clip_norm=1e9, global_batch_size=world_b, group=group, bucket=bucket)   # counters reset per step
            return torch.cat([p.detach().reshape(-1) for p in params])

        over = deep_step(s2, e2, dist.group.WORLD, 8, True)
        plain = deep_step(s2, e2, dist.group.WORLD, 8, False)
        alone = deep_step(0, 8, None, None, False)
        assert torch.equal(over, plain) and torch.allclose(over, alone, atol=1e-6)
        ragged = deep_step(s2, e2, dist.group.WORLD, 8, True, skip_mid=(rank == 1))
        both = [torch.zeros_like(ragged) for _ in range(world)]
        dist.all_gather(both, ragged)
        assert torch.equal(both[0], both[1])
        # overlap mode takes ONE backward per zero_(): a second one would add local gradients into ranges that are already summed across
        # ranks (the replicas would drift apart silently) - it must raise instead
        model = _Deep(False)
        params = list(model.parameters())
        bucket = parallel.GradBucket(params).enable_overlap(dist.group.WORLD, segments=3)
        bucket.zero_()
        x = xs[s2:e2]
        model([type("PB", (), {"x": x})()], True)["log_probability"].sum().backward()
        raised = False
        try:
            model([type("PB", (), {"x": x})()], True)["log_probability"].sum().backward()
        except RuntimeError as exc:
            raised = "one backward per step" in str(exc)
        bucket.allreduce(dist.group.WORLD)                  # (every rank issued the same collectives before raising: nothing is left unpaired)
        assert raised, "a second backward in overlap mode must raise"
        out.put((rank, "ok"))
    except Exception as exc:  # pragma: no cover
        out.put((rank, repr(exc)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    results = [out.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


def _bench(args, env_extra):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DFOL_BENCH_SHARE_GPU"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=env, cwd=root, capture_output=True, text=True, timeout=300)


def test_bench_refuses_a_world_size_mismatch():
    """bench.py --gpus N must never print a line for a different world size (round-1 finding: the flag was ignored)."""
    r = _bench(["--gpus", "2", "--steps", "1"], {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_launcher_needs_the_gpus_it_is_asked_for():
    """Without a launcher, --gpus 2 starts its own ranks - and says so loudly when the box has fewer GPUs (none here)."""
    if torch.cuda.device_count() >= 2:
        return
    r = _bench(["--gpus", "2", "--steps", "1"], {})
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr


def test_bench_plain_and_full_options():
    """A plain run is the headline only; --full turns the other legs on; --dump-outputs names the directory of the last step's outputs."""
    import bench
    a = bench.parse(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def test_bench_forward_outputs_as_float_arrays():
    """What a caller of the forward receives, as float arrays: binary answers as their index in ['no', 'yes'], open answers as their index
    among the question's own options, flattened with a count per question."""
    import bench
    res = {"log_probability": torch.tensor([-0.1, -2.0, -0.5]), "answer": [["yes"], ["no"], ["yes"]], "options": ["no", "yes"],
           "answer_log_probability": [[-0.1], [-0.14], [-0.5]], "type": QuestionType.BINARY}
    out = bench.forward_outputs(res)
    assert out["log_probability"].dtype == np.float32 and out["log_probability"].tolist() == res["log_probability"].tolist()
    assert out["answer_index"].tolist() == [1, 0, 1] and out["answer_count"].tolist() == [1, 1, 1]
    assert out["answer_log_probability"].dtype == np.float64 and np.allclose(out["answer_log_probability"], [-0.1, -0.14, -0.5])
    q = {"log_probability": torch.tensor([-1.0, -3.0], dtype=torch.float64), "answer": [["red", "blue"], ["big"]],
         "options": [["blue", "red"], ["small", "large"]], "answer_log_probability": [[-1.0, -1.2], [-3.0]], "type": QuestionType.QUERY}
    out = bench.forward_outputs(q)
    assert out["log_probability"].dtype == np.float64
    assert out["answer_index"].tolist() == [1, 0, -1] and out["answer_count"].tolist() == [2, 1]
    train = bench.forward_outputs({"log_probability": torch.zeros(4, requires_grad=True), "answer": [], "type": QuestionType.BINARY})
    assert list(train) == ["log_probability"]


def test_bench_dump_outputs_stays_within_its_budget(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files (integers and 16-bit floats widen); an array over its share of the budget keeps a
    seeded sample of its entries, the same in every run; ranks > 0 write <name>.rank<r>.npy."""
    import bench
    big = torch.arange(100000, dtype=torch.float32)
    arrays = {"small": torch.tensor([1, 2, 3]), "half": torch.ones(5, dtype=torch.bfloat16), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays, limit=40000)
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=40000)
    bench.dump_outputs(str(tmp_path / "r"), arrays, rank=1, world=2, limit=40000)
    small, half, b = (np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("small", "half", "big"))
    assert small.dtype == np.float64 and small.tolist() == [1, 2, 3] and half.dtype == np.float32 and half.tolist() == [1.0] * 5
    assert b.dtype == np.float32 and 0 < b.nbytes <= 40000 - small.nbytes - half.nbytes and b.size < big.numel()
    assert np.array_equal(b, np.load(str(tmp_path / "b" / "big.npy"))) and np.all(np.diff(b) > 0)
    assert sorted(os.listdir(str(tmp_path / "r"))) == ["big.rank1.npy", "half.rank1.npy", "small.rank1.npy"]
    assert np.load(str(tmp_path / "r" / "big.rank1.npy")).nbytes <= 20000

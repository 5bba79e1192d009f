"""DetectorTrainStep on two data-parallel ranks: two processes on the box's one card, gloo for the test (RCCL on a
real node - the same calls), ONE spawn.  Rank r runs micro-batch r of tests/test_gpu_detector_accum.py with that micro-batch's
generator; rank 1 starts from perturbed weights, so the broadcast at construction is what makes the replicas agree.

Every rank receives the same reduced bucket and decides from it, so parameters, both moments and the 40-byte state block are equal
across the ranks bit for bit after every step, skipped ones included; and since a two-operand fp32 sum is commutative the first step
equals the single-process ``accumulate=2`` update bit for bit.  Tensors are compared through their SHA-256 (equal digests: equal bits),
so that nothing of their size crosses the process boundary."""
import hashlib
import os
import socket
import traceback

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp          # noqa: E402

from layoutdit_amd import dp                # noqa: E402

LR = 1e-3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _params(model):
    return {k: _digest(v) for k, v in model.state_dict().items()}


def _snapshot(model, step):
    sd = step.state_dict()
    return {"params": _params(model), "exp_avg": {k: _digest(v) for k, v in sd["exp_avg"].items()},
            "exp_avg_sq": {k: _digest(v) for k, v in sd["exp_avg_sq"].items()}, "block": step._state.cpu().tolist(),
            "steps": sd["state"]["step"], "skipped": sd["state"]["skipped_steps"], "scale": sd["state"]["scale"]}


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from layoutdit_amd.training import DetectorTrainStep
    from tests import detector_accum_cases as cases
    r = dp.init(backend="gloo")
    try:
        m = cases.model()
        if rank == 1:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01)
        own = _params(m)
        step = DetectorTrainStep(m, lr=LR, init_scale=cases.SCALE, rank=r)
        out = {"own": own, "broadcast": _params(m), "steps": [], "losses": []}
        batches = cases.micro_batches()
        mine = batches[rank]
        for it in range(3):
            batch = cases.poisoned(mine) if (it == 2 and rank == 1) else mine
            losses = step.step(*batch, generator=cases.seeded(cases.GEN_SEEDS[rank]))
            torch.cuda.synchronize()
            out["steps"].append(_snapshot(m, step))
            out["losses"].append({k: float(v) for k, v in losses.items()})
        out["bucket"] = (step.bucket is not None, step.pending_micro_batches, step.iters)
        q.put((rank, out, None))
    except BaseException:
        q.put((rank, None, traceback.format_exc()))
        raise
    finally:
        dp.finalize(r)


def test_two_ranks_stay_identical_and_equal_the_accumulating_single_process():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(world):
            rank, out, err = q.get(timeout=300)
            assert err is None, f"rank {rank} failed:\n{err}"
            got[rank] = out
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    a, b = got[0], got[1]
    # the broadcast is what makes the replicas agree: rank 1 started elsewhere, both hold rank 0's weights afterwards
    assert a["own"] != b["own"] and a["broadcast"] == a["own"] and b["broadcast"] == a["own"]
    for it in range(3):
        for what in ("params", "exp_avg", "exp_avg_sq", "block", "steps", "skipped", "scale"):
            assert a["steps"][it][what] == b["steps"][it][what], (it, what)
    from tests import detector_accum_cases as cases
    assert [(s["steps"], s["skipped"], s["scale"]) for s in a["steps"]] == [(1, 0, cases.SCALE), (2, 0, cases.SCALE), (2, 1, cases.SCALE / 2)]
    assert a["steps"][0]["params"] != a["broadcast"] and a["steps"][1]["params"] != a["steps"][0]["params"]
    # the third step: rank 1 alone saw the infinities, both skipped, neither moved (parameters and moments), both halved the scale
    for what in ("params", "exp_avg", "exp_avg_sq"):
        assert a["steps"][2][what] == a["steps"][1][what] and b["steps"][2][what] == b["steps"][1][what], what
    assert a["bucket"] == b["bucket"] == (True, 0, 3)
    # the losses are each rank's own, not averaged: the ranks saw different pages
    assert a["losses"][0] != b["losses"][0]
    # one process, accumulate=2, the same two micro-batches with the same generators: the same update, bit for bit
    from layoutdit_amd.training import DetectorTrainStep
    m = cases.model()
    assert _params(m) == a["own"]
    single = DetectorTrainStep(m, lr=LR, init_scale=cases.SCALE, accumulate=2)
    batches = cases.micro_batches()
    for k in range(2):
        single.step(*batches[k], generator=cases.seeded(cases.GEN_SEEDS[k]))
    torch.cuda.synchronize()
    want = _snapshot(m, single)
    assert single.steps == 1
    for what in ("params", "exp_avg", "exp_avg_sq", "block"):
        assert want[what] == a["steps"][0][what], what

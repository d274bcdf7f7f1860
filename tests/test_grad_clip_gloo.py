"""CPU, world_size 2 over gloo: ShardedAdamW(max_grad_norm=...) combines the ranks' sums of squares (each rank sums ITS shards,
one all-reduce of the fp64 scalar) into the global norm, and clips with the factor every rank then agrees on."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_full_finetune_gloo import Tiny, _free_port, _loss


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from unsloth_amd.full_finetune import ShardedAdamW
    limit = 1e-2
    ids = torch.randint(0, 40, (2, 8), generator=torch.Generator().manual_seed(10 + rank))
    models, opts = [], []
    for mg in (limit, None):
        torch.manual_seed(0)
        models.append(Tiny().to(torch.bfloat16))
        opts.append(ShardedAdamW(models[-1], lr=3e-2, weight_decay=0.1, max_grad_norm=mg))
        _loss(models[-1], ids).backward()
        opts[-1].buckets.finish()
    B = opts[0].buckets
    [B.wait(bi) for bi in range(len(B.buckets))]
    # gloo all-reduces whole buckets: every rank can see the global gradient the shards are slices of
    ref = float(torch.stack([b["flat_g"].double().square().sum() for b in B.buckets]).sum().sqrt())
    opts[0].step()
    norm = float(opts[0].last_grad_norm)
    opts[1].step(grad_scale=float(torch.tensor(min(1.0, limit / (norm + 1e-6)), dtype=torch.float32)))
    same = all(torch.equal(p, r) for p, r in zip(models[0].parameters(), models[1].parameters()))
    q.put((rank, norm, ref, bool(same)))
    dist.destroy_process_group()


def test_sharded_clip_world2_sums_the_ranks_squares():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, n0, ref0, same0), (_, n1, ref1, same1) = res
    assert n0 == n1 and ref0 == ref1 and ref0 > 1e-2               # one norm for the group, above the limit
    assert abs(n0 - ref0) <= 2.0 ** -22 * ref0 and same0 and same1  # fp64 sums, one fp32 rounding; clipped == host factor

"""One rank of tests/test_gpu_slab.run_slabs run as a process of its own (slabs with peer stores or peer copies):
its own context on the z-slab it owns, the halo and all-reduce hooks served by wafer_amd.slab.HostStagedSlabComm (gloo, host
staging), the z-neighbours' buffers mapped through HIP IPC.  The body comes from the caller as a cloudpickle; the body's result
and the number of halo hook calls go back as a pickle.

    RANK=r WORLD_SIZE=w MASTER_ADDR=... MASTER_PORT=... python tests/slab_rank_worker.py JOB.pkl OUT.pkl"""
import dataclasses
import datetime
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import cloudpickle
    import torch
    import torch.distributed as dist
    import wafer_amd as wa
    from wafer_amd import slab

    job, out = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    with open(job, "rb") as f:
        base, body, connect = cloudpickle.load(f)
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    zb, zc = slab.partition(base.nz, world, rank)
    with wa.Context(dataclasses.replace(base, z_begin=zb, z_count=zc)) as ctx:
        comm = slab.HostStagedSlabComm(ctx, rank, world, dev)
        ctx.rendezvous = dist.barrier
        if connect or (connect is None and base.ext == 1 and base.halo_depth >= 3):
            if not slab.connect_peers(ctx, rank, world):
                raise SystemExit(f"rank {rank}: wafer_peer_connect failed")
        result = body(ctx, rank)
        ctx.synchronize()
        calls = comm.halo_calls
    with open(out, "wb") as f:
        pickle.dump((result, calls), f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

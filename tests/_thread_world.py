"""Several ranks of a slab decomposition as threads of one process, over the callback transport: what tests/test_distributed_gpu.py
and tests/_dist_iterates_script.py run the decomposed solve with on a box with one GPU.  The all-reduce adds the ranks' values in
rank order, on every rank alike: all ranks see the same bits."""


class _ThreadWorld:
    """A torch.distributed look-alike for several threads of one process, each playing one rank: the pieces
    DiffusionSolver uses (all_reduce on device tensors, P2POp / batch_isend_irecv of ghost planes).  A one-GPU box
    cannot host a multi-rank RCCL group (one rank per device), so this is how the N > 1 orchestration is run against
    the real HIP kernels -- slabs with live ghost planes, split SpMV, boundary-plane launches -- before the
    driver's multi-GPU run; RCCL itself is covered by the one-rank groups of tests/test_distributed_gpu.py and by torch."""

    def __init__(self, world, timeout=120):
        """timeout: seconds a rank waits for the others at a barrier or for a ghost plane before it gives up."""
        import queue
        import threading

        self.world, self.timeout = world, timeout
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.mail = {(a, b): queue.Queue() for a in range(world) for b in range(world)}

    def rank_view(self, rank):
        return _ThreadRank(self, rank)


class _ThreadRank:
    class ReduceOp:
        SUM = "sum"

    isend, irecv = "isend", "irecv"

    def __init__(self, world, rank):
        self.w, self.rank = world, rank

    def all_reduce(self, t, op=None, group=None):
        w = self.w
        self.reduces = getattr(self, "reduces", 0) + 1
        w.slots[self.rank] = t.clone()
        w.barrier.wait(timeout=w.timeout)
        total = w.slots[0].clone()
        for other in w.slots[1:]:
            total += other
        w.barrier.wait(timeout=w.timeout)  # everyone has read the slots before they are reused
        t.copy_(total)

    def P2POp(self, fn, tensor, peer, group=None):
        return (fn, tensor, peer)

    def get_global_rank(self, group, rank):
        return rank

    def batch_isend_irecv(self, ops):
        reqs = []
        for fn, tensor, peer in ops:
            if fn == self.isend:
                self.w.mail[(self.rank, peer)].put(tensor.clone())
            else:
                reqs.append(_ThreadRecv(self.w.mail[(peer, self.rank)], tensor, self.w.timeout))
        return reqs


class _ThreadRecv:
    def __init__(self, box, tensor, timeout=120):
        self.box, self.tensor, self.timeout = box, tensor, timeout

    def wait(self):
        self.tensor.copy_(self.box.get(timeout=self.timeout))


def _thread_solver(ops, slab, dist_view, loop):
    """DiffusionSolver of one thread-rank: ``loop="lib"`` runs beat_pde_solve_dist over a callback communicator whose
    transport is the thread world; ``loop="stage"`` the Python stage loop over the same world."""
    from beat._engine import DiffusionSolver, LibComm

    if dist_view is None:
        return DiffusionSolver(ops, slab)
    if loop == "lib":
        return DiffusionSolver(ops, slab, force_distributed=True, libcomm=LibComm(ops.ctx, slab, dist_view, None, "callbacks"))
    solver = DiffusionSolver(ops, slab, force_distributed=True, stage_driven=True)
    solver.dist = dist_view
    return solver

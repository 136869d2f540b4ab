"""GPU: the scalar steps the device runs are the ones the CPU tests hold (csrc/beat_pcg_scalar.h through pcg_step_kernel).  The stage
API drives Jacobi-PCG on two of the smallest shapes of tests/_pcg_ref.py; around every scalar step -- the start of the solve and each
roll -- the device's own state is read, and the plain g++ build of tests/pcg_scalar_harness.cpp, given the state before, must leave
bit for bit the state after: the device's sums go in, its decisions come out.  Division, comparison and negation are IEEE on both
sides, so there is no tolerance.  (Only the 16 host-visible slots are read: the predicted stop's arithmetic is held on the CPU, its
behaviour end to end by test_pcg_predicted_stop_gpu.py.)"""
import numpy as np
import pytest

import _oracle_ops as oo
import _pcg_ref as ref
from _pcg_scalar import Harness, build, same_bits

pytestmark = pytest.mark.gpu

DECIDED = [oo.ST_TOL2, oo.ST_BETA, oo.ST_RZ, oo.ST_RR, oo.ST_ITERS, oo.ST_STOP, oo.ST_REASON]
SHAPES = ((65, 3, 5), (2, 2, 2))
# run -> (v is zero, rtol, atol as a fraction of ||b||, max_it, reason, latched at begin)
RUNS = {
    "rtol": (False, 1e-9, 0.0, ref.KMAX, 2, False),
    "atol": (False, 1e-12, 1e-3, ref.KMAX, 3, False),
    "cut": (False, 1e-12, 0.0, 2, -3, False),
    "zero": (True, 1e-9, 0.0, ref.KMAX, 2, True),
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    h = Harness(build(tmp_path_factory.mktemp("pcg_scalar_harness"), "plain"))
    yield h
    h.close()


@pytest.fixture
def multi_launch():
    from beat._engine import HipOps

    old = HipOps.default_small
    HipOps.default_small = False
    yield
    HipOps.default_small = old


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("shape", SHAPES, ids=ref.shape_key)
def test_device_steps_equal_the_header_on_the_host(hip_ctx, harness, multi_launch, shape, run):
    from beat._engine import HipOps

    zero, rtol, atol_rel, max_it, reason, at_begin = RUNS[run]
    p = ref.problem(shape)
    ops = HipOps(hip_ctx, shape, True, True, p.mass_tab, p.stiff_tab)
    ops.set_timestep(ref.C_M, ref.THETA, ref.DT)
    v, x = ops.new_field(), ops.new_field()
    v.set(np.zeros(p.n) if zero else ref.field(shape))

    def held(step, device_step):
        """Run a scalar step on the device and on the host, from the device's state before it."""
        before = ops.read_state()
        device_step()
        after = ops.read_state()
        harness.set(np.concatenate([before, np.zeros(16)]))
        host, _ = step()
        assert same_bits(host[DECIDED], after[DECIDED]), (shape, run, before, after, host[:16])
        return after

    ops.rhs(v, [], [], x)
    atol = atol_rel * float(np.sqrt(ops.read_state()[oo.ST_BB]))
    st = held(lambda: harness.begin(rtol, atol, max_it), lambda: ops.cg_begin(rtol, atol, max_it))
    assert (st[oo.ST_STOP] != 0.0) == at_begin
    ring, i = len(ops.ring), 0
    while st[oo.ST_STOP] == 0.0 and i <= ref.KMAX:
        cur, nxt = ops.ring[i % ring], ops.ring[(i + 1) % ring]
        ops.p = cur
        ops.spmv_dot()
        ops.cg_update_r(i % ring)
        st = held(harness.roll, lambda: ops.cg_next_oop(cur, nxt))
        i += 1
    assert st[oo.ST_STOP] == 1.0 and st[oo.ST_REASON] == reason and st[oo.ST_ITERS] == i, (shape, run, st)
    assert same_bits(held(harness.roll, lambda: ops.cg_next_oop(ops.ring[0], ops.ring[1])), st)  # latched: a roll changes nothing

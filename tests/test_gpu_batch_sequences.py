"""Random call sequences on one long-lived wafer_amd.Batch on the MI355X (tests/batch_sequences.py).  The feature tests each start
from a fresh batch; here about forty calls of every kind follow one another in an order nobody wrote down, as wafer_amd/sweep.py
uses a batch, and after every call every member's whole state (phi, V, pot_sub, every stored state, the counts, the call's return
value) is compared with

  T1  the same member alone in a Batch of one, given the projection of the program onto it      every dtype, byte for byte
  T2  a free-running Context of its Params (programs without excited-state arithmetic)           every dtype, byte for byte
  T3  the CPU oracle, loaded with what the device held before the call                           f64, the suite's existing bars

so that a Gram matrix, a member table, a workgroup table or a view flag that one call forgot to bring up to date shows at the call
that reads it.  tests/test_batch_sequences_host.py checks on the CPU that these seeds reach the transitions where that can happen.
A failure prints the seed, the op and the program up to it; `python -m tests.batch_sequences --seed N --kind K` prints a program."""
import pytest

pytestmark = pytest.mark.gpu

from tests import batch_sequences as bs  # noqa: E402

CASES = [(seed, kind, ext, dtype) for kind in bs.KINDS for seed in bs.SEEDS[kind] for ext in bs.EXTS for dtype in bs.DTYPES]


@pytest.fixture(scope="module")
def wo():
    from oracle import wafer_oracle
    wafer_oracle.build()
    return wafer_oracle


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


@pytest.mark.parametrize("seed,kind,ext,dtype", CASES, ids=["%s-seed%d-ext%d-%s" % (k, s, e, d) for s, k, e, d in CASES])
def test_sequence(wa, wo, seed, kind, ext, dtype):
    n_ops, n_refused = bs.check_case(wa, wo, (seed, kind, ext, dtype))
    print("%s seed %d ext %d %s: %d ops, %d of them refused" % (kind, seed, ext, dtype, n_ops, n_refused))
    assert n_ops >= bs.N_OPS

"""Member addressing of a one-shape batch on the MI355X.  Every batched kernel takes what depends on the member -- its partition,
its workgroup count, where its partials begin, its origin in a store slot -- from its WaferBatchMember record, for one shape as for
several.  In a batch of one member every such offset is 0; in a wafer_batch_create batch of three, members 1 and 2 sit at
obs_off = m * 4 * obs_nb, n2_off = m * n2_nb, gs_off = m * gs_nb and slot_off = m * total + base_off.  Independence of B, index and
active set is the documented contract, so each member of the three must be, byte for byte, the same member alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import make_pair, random_phi  # noqa: E402

# two 64-wide x tiles, a ragged 4-row y tile, nz below one 4-plane chunk; SevenPoint so that symmetrise runs
SHAPE, EXT, WNUM = (65, 13, 3), 3, 2
SPECS = [dict(dn=0.2, dt=0.004, mass=1.0), dict(dn=0.2, dt=0.003, mass=1.0), dict(dn=0.2, dt=0.0055, mass=1.0)]
CONS = ["AboutZ", "AntisymAboutY", "AboutY"]
FROZEN_FIRST = [0, 1, 1]


@pytest.fixture(scope="module")
def wa():
    import wafer_amd
    wafer_amd.load_library()
    return wafer_amd


def member(k, dtype):
    """(par, phi, states) of member k: its own dt and start; two stored states shared by nobody"""
    cfg, par = make_pair(SHAPE, ext=EXT, potential="Harmonic", dtype=dtype, **SPECS[k])
    phi = random_phi(cfg, seed=70 + k)
    states = [random_phi(cfg, seed=170 + 10 * k + l) / np.sqrt(np.prod(SHAPE)) for l in range(WNUM)]
    return par, phi, states


def bits(x):
    if isinstance(x, dict):
        x = [x[k] for k in sorted(x)]
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes()


def run(wa, ks, dtype, source):
    """the sequence under test on a wafer_batch_create batch of the members ks -> {stage: [bytes per member]}"""
    out = {}
    with wa.Batch([member(k, dtype)[0] for k in ks]) as b:
        assert b.num_shapes() == 1 and "shapes" not in b.dispatch()
        for slot, k in enumerate(ks):
            par, phi, states = member(k, dtype)
            b.set_potential(slot, "Harmonic")
            b.upload_phi(slot, phi)
            for l, s in enumerate(states):
                b.load_state(slot, l, s)

        def phis():
            return [bits(b.download_phi(slot)) for slot in range(len(ks))]
        out["observables"] = [bits(o) for o in b.observables()]
        n2 = b.norm2()
        out["norm2"] = [bits(x) for x in n2]
        b.normalise(n2)
        out["normalise"] = phis()
        b.symmetrise([CONS[k] for k in ks])
        out["symmetrise"] = phis()
        b.resample_phi(source)
        out["resample_phi"] = phis()
        for active in (None, [FROZEN_FIRST[k] for k in ks]):
            for variant in (0, 1):
                b.set_gs_variant(variant)
                b.evolve(3, wnum=WNUM, active=active)
                assert b.gs_dispatch(WNUM)["form"] == ("onepass" if variant else "sequential")
                out["evolve gs_variant=%d active=%s" % (variant, "all" if active is None else FROZEN_FIRST)] = phis()
        out["observables after"] = [bits(o) for o in b.observables()]
        out["norm2 after"] = [bits(x) for x in b.norm2()]
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_each_member_of_three_is_the_member_alone(wa, dtype):
    source = np.random.default_rng(5).standard_normal((5, 5, 5))
    three = run(wa, [0, 1, 2], dtype, source)
    for k in range(3):
        alone = run(wa, [k], dtype, source)
        assert list(alone) == list(three)
        for stage in three:
            assert three[stage][k] == alone[stage][0], (dtype, k, stage)
    # the members differ, so equal bytes are not three copies of one answer (but for resample_phi: one source onto one shape gives
    # every member the same array, from which their dt and stores part them again), and the frozen member kept its bits
    for stage in three:
        assert len(set(three[stage])) == (1 if stage == "resample_phi" else 3), stage
    assert three["evolve gs_variant=0 active=%s" % FROZEN_FIRST][0] == three["evolve gs_variant=1 active=all"][0]
    assert three["evolve gs_variant=1 active=%s" % FROZEN_FIRST][0] == three["evolve gs_variant=1 active=all"][0]
    assert three["evolve gs_variant=1 active=%s" % FROZEN_FIRST][1] != three["evolve gs_variant=1 active=all"][1]

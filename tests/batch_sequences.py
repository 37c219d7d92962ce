"""Model-based sequence tests of wafer_amd.Batch: seeded random programs of Batch calls, their executors and a CPU model.

A Batch keeps a lot of state between calls by hand (the Gram matrices of the one-pass form, the device copy of the member table,
the two workgroup tables, each view's flags, buffers made at first use), and the feature tests each start from a fresh batch.  Here
one long-lived batch takes about forty calls in an order nobody wrote down, and after EVERY call each member's whole state -- phi, V,
pot_sub, every stored state, the counts, the call's own return value -- is compared with

  T1  the same member alone in a Batch([par]) given the projection of the program onto it       (every dtype; byte for byte)
  T2  a free-running Context of its Params, for programs without excited-state arithmetic        (every dtype; byte for byte)
  T3  HostModel below, the CPU oracle, loaded with what the device held BEFORE the call           (f64; the suite's own bars)

program() is a pure function of its arguments; `python -m tests.batch_sequences --seed N --kind K --ext E` prints one (CPU only).
tests/test_batch_sequences_host.py checks on the CPU that the committed seeds reach the transitions the caches can get wrong;
tests/test_gpu_batch_sequences.py runs them on the device.  No test lives in this file."""
from __future__ import annotations

import argparse
import dataclasses
import struct

import numpy as np

KINDS = ("one_shape", "mixed", "mixed_states")
# two members share a shape; (65, 13, 3): two 64-wide x tiles, a ragged y tile, nz below one z chunk
SHAPES = [(20, 13, 9), (65, 13, 3), (20, 13, 9), (33, 8, 12), (12, 16, 7)]
SEEDS = {kind: [0, 1, 2, 3, 4, 5] for kind in KINDS}
N_OPS = 40
DTYPES = ("f64", "f32", "f32fast")
EXTS = (1, 2, 3)   # ext 3 (SevenPoint) is where symmetrise runs
ALGEBRAIC = ("Harmonic", "Coulomb", "SimpleCornell", "Cube", "NoPotential")   # + - * / sqrt only: the oracle's V bit for bit
CLOSED_FORM = ("Harmonic", "Coulomb", "SimpleCornell")                        # re-evaluated by the excited-state kernels
ICS = ("Constant", "Boolean", "Gaussian")
CONSTRAINTS = ("NotConstrained", "AboutZ", "AntisymAboutZ", "AboutY", "AntisymAboutY")
EVOLVE_STEPS = (1, 2, 3, 4, 5, 7)
WAFER_OK, WAFER_ERR_INVALID, WAFER_ERR_STATE, WAFER_ERR_MAX_STEP = 0, -1, -4, -5

STORE_CHANGES = ("push_state", "load_state", "resample_state", "rotate_states", "clear_states", "ritz", "solve_state")
PHI_WRITERS = ("symmetrise", "clone_state_to_phi", "upload_phi", "resample_phi")


def seed_ext(seed):
    return 1 + seed % 3


def ground_only(seed, kind):
    """programs without excited-state arithmetic (evolve with wnum > 0, orthogonalise, solve_state above 0): held to Contexts"""
    return kind == "mixed" or seed % 6 in (2, 3)


def fused_steps(ext):
    """K of the fused ground-state pass (wafer_engine_batch.hip: steps_per_pass)"""
    return 3 if ext == 1 else 2


# ---- members ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Member:
    shape: tuple
    dn: float
    dt: float
    mass: float
    max_states: int


def members(seed, kind, ext):
    """about five small, awkward members, each with its own dt, dn and mass; max_states 5 on seeds 1 and 4 (wnum 5 has no one-pass
    form and takes the sequential one)"""
    rng = np.random.default_rng([seed, KINDS.index(kind), ext, 1])
    shapes = [SHAPES[(seed + ext) % len(SHAPES)]] * 5 if kind == "one_shape" else list(SHAPES)
    out = []
    for shape in shapes:
        dn = float(rng.choice([0.2, 0.25, 0.3]))
        mass = float(rng.choice([0.5, 1.0, 1.5, 2.0]))
        # dt <= dn^2 / 3 (config.rs:363) is the reference's check; the explicit step is stable for dt < m dn^2 / 3 on the ThreePoint
        # stencil and two thirds of that on the SevenPoint one -- a program must not grow its norms by orders of magnitude
        dt = float(np.round(dn * dn * min(mass, 1.0) * rng.uniform(0.04, 0.18), 5))
        out.append(Member(tuple(shape), dn, dt, mass, 5 if seed % 3 == 1 else 4))
    return out


def params_of(wa, mem, ext, dtype):
    return wa.Params(*mem.shape, dn=mem.dn, dt=mem.dt, mass=mem.mass, central_difference=ext, dtype=dtype, max_states=mem.max_states)


def config_of(wo, mem, ext, potential="Harmonic"):
    return wo.Config(*mem.shape, ext=ext, potential=potential, dn=mem.dn, dt=mem.dt, mass=mem.mass)


def padded(shape, ext):
    return tuple(n + 2 * ext for n in shape)


# ---- ops -------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Op:
    """one Batch call: its name, its keyword arguments, its mask (None: every member) and, for a call that must be refused, the
    WaferError code.  Arrays are specs -- ("normal", seed, shape, scale) or ("frame0", seed, work shape, ext, scale) -- so that a
    program prints on one screen; materialise() makes them."""
    name: str
    kw: tuple = ()
    active: tuple | None = None
    refused: int | None = None

    def __getitem__(self, key):
        return dict(self.kw)[key]

    def get(self, key, default=None):
        return dict(self.kw).get(key, default)

    def __repr__(self):
        def short(v):
            return "<array %s>" % (v.shape,) if isinstance(v, np.ndarray) else repr(v)
        parts = ["%s=%s" % (k, short(v)) for k, v in self.kw]
        if self.active is not None:
            parts.append("active=%s" % (list(self.active),))
        if self.refused is not None:
            parts.append("REFUSED=%d" % self.refused)
        return "%s(%s)" % (self.name, ", ".join(parts))


def mk(name, active=None, refused=None, **kw):
    return Op(name, tuple(kw.items()), None if active is None else tuple(int(x) for x in active), refused)


def materialise(spec):
    if spec is None or isinstance(spec, np.ndarray):
        return spec
    if spec[0] == "normal":
        _, seed, shape, scale = spec
        return np.ascontiguousarray(np.random.default_rng(seed).standard_normal(shape) * scale)
    if spec[0] == "frame0":   # work cells ~ N(0, scale^2) in a zero Dirichlet frame
        _, seed, shape, ext, scale = spec
        out = np.zeros(padded(shape, ext))
        out[ext:-ext, ext:-ext, ext:-ext] = np.random.default_rng(seed).standard_normal(shape) * scale
        return out
    if spec[0] == "rot":      # a well-conditioned (k, k) matrix: the identity plus at most 0.25 per entry
        _, seed, k = spec
        return np.eye(k) + np.random.default_rng(seed).uniform(-0.25, 0.25, (k, k))
    raise ValueError("unknown array spec %r" % (spec,))


def listed(op, B):
    """the members a masked op names"""
    return [m for m in range(B) if op.active is None or op.active[m]]


PER_MEMBER = ("set_potential", "set_potential_host", "set_potsub", "set_initial_condition", "upload_phi", "load_state")
MASKED = ("set_potentials", "set_initial_conditions", "resample_phi", "resample_potential", "resample_potsub", "resample_state",
          "symmetrise", "evolve", "normalise", "orthogonalise", "push_state", "clear_states", "clone_state_to_phi", "ritz_matrices",
          "rotate_states", "ritz")
EVERYONE = ("norm2", "observables", "solve", "solve_state", "set_step_variant", "set_gs_variant")
STATE_CALLS = ("load_state", "resample_state", "orthogonalise", "push_state", "clear_states", "clone_state_to_phi", "solve_state")
OP_NAMES = PER_MEMBER + MASKED + EVERYONE


def touched(op, B):
    """the members whose state or return value a (valid) op concerns"""
    if op.name in PER_MEMBER:
        return [op["i"]]
    if op.name in MASKED:
        return listed(op, B)
    return list(range(B))


# ---- the generator's bookkeeping: what makes an op valid -------------------------------------------------------------------------------
class Book:
    """each member's state count, whether it has phi and V, the batch's variants: enough to say of any op whether the library takes it"""

    def __init__(self, mems, kind, ext):
        self.mems, self.kind, self.ext, self.B = mems, kind, ext, len(mems)
        self.nst = [0] * self.B
        self.cap = [m.max_states for m in mems]
        self.have_pot = [False] * self.B
        self.have_phi = [False] * self.B
        self.in_store = [False] * self.B   # phi is a copy of one of the member's stored states
        self.unit = [False] * self.B       # phi has norm2 about 1, as a state in a store should
        self.norm_fresh = [False] * self.B # the norm last read is the norm of phi as it stands
        self.step_variant, self.gs_variant = -1, -1
        self.have_norm2 = False
        self.stores = kind != "mixed"

    def why_invalid(self, op):
        """None for a call the library takes, else the reason it refuses it"""
        n, B = op.name, self.B
        act = touched(op, B)
        if not self.stores and (n in STATE_CALLS or (n == "evolve" and op["wnum"]) or (n == "set_gs_variant" and op["variant"] == 1)):
            return "a state call on a mixed-shape batch without state stores"
        src = op.get("src")
        if isinstance(src, tuple) and src[0] in ("member", "state"):
            if src[0] == "state" and not self.stores:
                return "a stored state as the source on a mixed-shape batch without state stores"
            if src[1] in act:   # (stricter than the library: it refuses only the same buffer as source and target)
                return "the source member is among the targets"
            if src[0] == "member" and not self.have_phi[src[1]]:
                return "the source member has no phi"
            if src[0] == "state" and src[2] >= self.nst[src[1]]:
                return "the source member has no such state"
        need_phi = n in ("symmetrise", "evolve", "normalise", "orthogonalise", "push_state", "norm2", "observables", "solve", "solve_state")
        need_pot = n in ("evolve", "observables", "solve", "solve_state", "set_potsub", "resample_potsub", "ritz_matrices", "ritz")
        for m in act:
            if need_phi and not self.have_phi[m]:
                return "member %d has no phi" % m
            if need_pot and not self.have_pot[m]:
                return "member %d has no potential" % m
        if n in ("evolve", "orthogonalise") and any(op["wnum"] > self.nst[m] for m in act):
            return "wnum above a member's store"
        if n == "solve_state" and any(op["wnum"] > self.nst[m] or self.nst[m] >= self.cap[m] for m in act):
            return "solve_state needs wnum states and room for the result in every store"
        if n == "solve" and self.stores and any(self.nst[m] >= self.cap[m] for m in act):
            return "a Context's solve pushes its result: every store needs room"   # (the batch would take it; run_contexts could not follow)
        if n == "push_state" and any(self.nst[m] >= self.cap[m] for m in act):
            return "a full store"
        if n in ("load_state", "resample_state") and any(op["idx"] > self.nst[m] or op["idx"] >= self.cap[m] for m in act):
            return "states are loaded in order, up to max_states"
        if n == "clone_state_to_phi" and any(op["idx"] >= self.nst[m] for m in act):
            return "no such state"
        if n in ("ritz_matrices", "ritz") and any(not 1 <= op["ks"][m] <= self.nst[m] for m in act):
            return "k outside 1 .. the member's state count"
        if n == "rotate_states" and any(not 1 <= op["coefs"][m][2] <= self.nst[m] for m in act):
            return "k outside 1 .. the member's state count"
        if n == "symmetrise" and self.ext != 3 and any(op["constraints"][m] != "NotConstrained" for m in act):
            return "symmetry constraints need the SevenPoint frame"
        if n == "normalise" and not self.have_norm2:
            return "no norms read yet"
        return None

    def commit(self, op):
        """the bookkeeping of a call the library took"""
        n = op.name
        act = touched(op, self.B)
        for m in act:
            if n in ("set_initial_condition", "set_initial_conditions", "upload_phi", "resample_phi", "symmetrise"):
                self.unit[m] = False
            if n in ("clone_state_to_phi", "solve", "solve_state") or (n == "evolve" and op["wnum"]):
                self.unit[m] = True    # an excited step normalises; so does every block of a solve; a stored state is kept at norm 1
            if n == "normalise":
                self.unit[m] = self.norm_fresh[m]
            if n in ("set_initial_condition", "set_initial_conditions", "upload_phi", "resample_phi", "symmetrise", "evolve", "normalise",
                     "orthogonalise", "clone_state_to_phi", "solve", "solve_state"):
                self.norm_fresh[m] = False
            if n in ("set_potential", "set_potentials", "set_potential_host", "resample_potential"):
                self.have_pot[m] = True
            if n in ("set_initial_condition", "set_initial_conditions", "upload_phi", "resample_phi", "clone_state_to_phi"):
                self.have_phi[m] = True
            if n in ("set_initial_condition", "set_initial_conditions", "upload_phi", "resample_phi", "evolve", "solve"):
                self.in_store[m] = False
            if n in ("push_state", "clone_state_to_phi"):
                self.in_store[m] = True
            if n == "push_state":
                self.nst[m] += 1
            if n in ("load_state", "resample_state"):
                self.nst[m] = max(self.nst[m], op["idx"] + 1)
            if n == "clear_states":
                self.nst[m] = 0
        if n == "set_step_variant":
            self.step_variant = op["variant"]
        if n == "set_gs_variant":
            self.gs_variant = op["variant"]
        if n == "norm2":
            self.have_norm2 = True
            self.norm_fresh = [True] * self.B

    def after_solve_state(self, converged):
        """solve_state pushes the members that converged: only a run tells which"""
        for m in range(self.B):
            if converged[m]:
                self.nst[m] += 1
                self.in_store[m] = True
            else:
                self.in_store[m] = False


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed, kind, ext, n_ops):
        self.rng = np.random.default_rng([seed, KINDS.index(kind), ext, 2])
        self.seed, self.kind, self.ext, self.n_ops = seed, kind, ext, n_ops
        self.mems = members(seed, kind, ext)
        self.B = len(self.mems)
        self.book = Book(self.mems, kind, ext)
        self.excited = not ground_only(seed, kind)
        self.ops = []
        self.n_refused = 0
        self.K = fused_steps(ext)

    # -- draws ------------------------------------------------------------------------------------------------------------------------------
    def aseed(self):
        return int(self.rng.integers(1, 10 ** 6))

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def mask(self, ok=None, allow_none=True, proper=False):
        """a random mask over the members for which ok(m) holds: None (everyone, where everyone may), one member, or some; proper: never
        everyone.  Returns False where nobody may."""
        can = [m for m in range(self.B) if ok is None or ok(m)]
        if not can:
            return False
        r = self.rng.random()
        if len(can) == self.B and allow_none and not proper and r < 0.3:
            return None
        if r < 0.5 or len(can) == 1:
            chosen = [self.pick(can)]
        else:
            chosen = [m for m in can if self.rng.random() < 0.6] or [self.pick(can)]
            if proper and len(chosen) == self.B:
                chosen = chosen[:-1]
        if proper and len(chosen) == self.B:
            return False
        return tuple(1 if m in chosen else 0 for m in range(self.B))

    def members_of(self, mask):
        return [m for m in range(self.B) if mask is None or mask[m]]

    def emit(self, op):
        """append a valid op (False if the library would refuse it)"""
        if self.book.why_invalid(op) is not None:
            return False
        self.ops.append(op)
        self.book.commit(op)
        return True

    def phi_spec(self, m):
        return ("frame0", self.aseed(), self.mems[m].shape, self.ext, float(self.pick([1.0, 0.5, 0.02])))

    def state_spec(self, m):   # norm2 about 1, as a converged state's
        return ("frame0", self.aseed(), self.mems[m].shape, self.ext, float(1.0 / np.sqrt(np.prod(self.mems[m].shape))))

    def source(self, states=True, avoid=(), scale=1.0, unit=False):
        """a small numpy source, or a member's phi / stored state on the device (never a member of `avoid`; unit: only a phi of norm 1)"""
        b, r = self.book, self.rng.random()
        free = [m for m in range(self.B) if m not in avoid]
        if r < 0.25:
            have = [m for m in free if b.have_phi[m] and (b.unit[m] or not unit)]
            if have:
                return ("member", self.pick(have))
        elif r < 0.4 and states and b.stores:
            have = [m for m in free if b.nst[m] > 0]
            if have:
                m = self.pick(have)
                return ("state", m, int(self.rng.integers(b.nst[m])))
        return ("normal", self.aseed(), self.pick([(2, 2, 2), (5, 4, 3), (9, 6, 5), (24, 15, 11)]), scale)

    # -- single ops -------------------------------------------------------------------------------------------------------------------------
    def e_set_potential(self):
        return self.emit(mk("set_potential", i=int(self.rng.integers(self.B)), pot=self.pick(ALGEBRAIC)))

    def e_set_potentials(self, mask=0):
        mask = self.mask() if mask == 0 else mask
        return self.emit(mk("set_potentials", active=mask, names=tuple(self.pick(ALGEBRAIC) for _ in range(self.B))))

    def e_set_potential_host(self, i=None):
        i = int(self.rng.integers(self.B)) if i is None else i
        kind = int(self.pick([0, 0, 1, 2]))
        sub = ("normal", self.aseed(), self.mems[i].shape, 1.0) if kind == 2 else None
        return self.emit(mk("set_potential_host", i=i, v=("normal", self.aseed(), padded(self.mems[i].shape, self.ext), 1.0),
                            potsub_kind=kind, potsub_scalar=float(np.round(self.rng.uniform(-2, 2), 3)) if kind == 1 else 0.0, potsub=sub))

    def e_set_potsub(self, i=None, kind=None):
        i = int(self.rng.integers(self.B)) if i is None else i
        kind = int(self.rng.integers(3)) if kind is None else kind
        sub = ("normal", self.aseed(), self.mems[i].shape, 1.0) if kind == 2 else None
        return self.emit(mk("set_potsub", i=i, kind=kind, scalar=float(np.round(self.rng.uniform(-2, 2), 3)), potsub=sub))

    def e_set_initial_condition(self):
        return self.emit(mk("set_initial_condition", i=int(self.rng.integers(self.B)), ic=self.pick(ICS), seed=int(self.rng.integers(100))))

    def e_set_initial_conditions(self, mask=0):
        mask = self.mask() if mask == 0 else mask
        return self.emit(mk("set_initial_conditions", active=mask, names=tuple(self.pick(ICS) for _ in range(self.B)),
                            seeds=tuple(int(self.rng.integers(100)) for _ in range(self.B))))

    def e_upload_phi(self, i=None):
        i = int(self.rng.integers(self.B)) if i is None else i
        return self.emit(mk("upload_phi", i=i, phi=self.phi_spec(i)))

    def e_resample_phi(self, mask=0):
        mask = self.mask(proper=self.rng.random() < 0.5) if mask == 0 else mask
        if mask is False:
            return False
        avoid = self.members_of(mask)
        return self.emit(mk("resample_phi", active=mask, src=self.source(avoid=avoid), basis=self.pick(["padded", "work"])))

    def e_resample_potential(self, mask=0):
        mask = self.mask() if mask == 0 else mask
        src = ("normal", self.aseed(), self.pick([(2, 2, 2), (5, 4, 3), (9, 6, 5)]), 1.0)   # V from a wavefunction is legal, and dull
        return self.emit(mk("resample_potential", active=mask, src=src, basis=self.pick(["padded", "work"])))

    def e_resample_potsub(self):
        return self.emit(mk("resample_potsub", active=self.mask(), src=("normal", self.aseed(), self.pick([(3, 3, 3), (9, 6, 5)]), 1.0), basis="work"))

    def e_resample_state(self, mask=0):
        b = self.book
        if not b.stores:
            return False
        idx = int(self.rng.integers(0, 1 + min(max(b.nst), min(b.cap) - 1)))
        mask = self.mask(lambda m: idx <= b.nst[m] and idx < b.cap[m], proper=self.rng.random() < 0.5) if mask == 0 else mask
        if mask is False:
            return False
        src = self.source(avoid=self.members_of(mask), scale=0.03, unit=True)   # a few thousand cells: norm2 about 1
        return self.emit(mk("resample_state", active=mask, idx=idx, src=src, basis="padded" if src[0] != "normal" else self.pick(["padded", "work"])))

    def e_symmetrise(self, mask=0):
        if self.ext != 3:
            return False
        mask = self.mask() if mask == 0 else mask
        return self.emit(mk("symmetrise", active=mask, constraints=tuple(self.pick(CONSTRAINTS) for _ in range(self.B))))

    def e_evolve(self, mask=0, wnum=None, steps=None):
        b = self.book
        mask = self.mask() if mask == 0 else mask
        if mask is False:
            return False
        top = min(b.nst[m] for m in self.members_of(mask)) if (self.excited and b.stores) else 0
        if wnum is None:
            wnum = int(self.rng.integers(0, top + 1)) if self.rng.random() < 0.7 else 0
        steps = int(self.pick(EVOLVE_STEPS)) if steps is None else steps
        return self.emit(mk("evolve", active=mask, steps=steps, wnum=int(wnum)))

    def e_excited_evolve(self, mask=0, steps=None):
        b = self.book
        if not (self.excited and b.stores):
            return False
        mask = self.mask(lambda m: b.nst[m] >= 1) if mask == 0 else mask
        if mask is False:
            return False
        top = min(b.nst[m] for m in self.members_of(mask))
        return top >= 1 and self.e_evolve(mask, int(self.rng.integers(1, top + 1)), steps)

    def e_set_step_variant(self):
        return self.emit(mk("set_step_variant", variant=int(self.rng.integers(2))))

    def e_set_gs_variant(self):
        if not self.book.stores:
            return False
        v = int(self.rng.integers(2))
        if v == 1 and self.book.gs_variant != 1 and self.excited:
            return self.m_first_onepass()
        return self.emit(mk("set_gs_variant", variant=v))

    def e_norm2(self):
        return self.emit(mk("norm2"))

    def e_normalise(self):
        return self.emit(mk("normalise", active=self.mask()))

    def e_orthogonalise(self, mask=0):
        b = self.book
        if not (self.excited and b.stores):
            return False
        # (a phi that is a copy of a stored state would be projected to rounding noise, which no two implementations share)
        mask = self.mask(lambda m: b.nst[m] >= 1 and not b.in_store[m]) if mask == 0 else mask
        if mask is False or any(b.in_store[m] for m in self.members_of(mask)):
            return False
        top = min(b.nst[m] for m in self.members_of(mask))
        return top >= 1 and self.emit(mk("orthogonalise", active=mask, wnum=int(self.rng.integers(1, top + 1))))

    def e_push_state(self, mask=0):
        b = self.book
        # (a second copy of one phi in a store makes it linearly dependent: Rayleigh-Ritz refuses it, Gram-Schmidt is 0 / 0)
        mask = self.mask(lambda m: b.nst[m] < b.cap[m] and not b.in_store[m]) if mask == 0 else mask
        if mask is False or not b.stores or any(b.in_store[m] for m in self.members_of(mask)):
            return False
        self.make_unit(mask)
        return self.emit(mk("push_state", active=mask))

    def make_unit(self, mask):
        """the listed members' phi at norm 1 before it goes to a store: norm2 and normalise, where it is not already"""
        if any(not self.book.unit[m] for m in self.members_of(mask)):
            self.e_norm2()
            self.emit(mk("normalise", active=mask))

    def e_load_state(self, i=None, idx=None):
        b = self.book
        if not b.stores:
            return False
        i = int(self.rng.integers(self.B)) if i is None else i
        if idx is None:
            idx = int(self.rng.integers(0, min(b.nst[i], b.cap[i] - 1) + 1))
        return self.emit(mk("load_state", i=i, idx=int(idx), state=self.state_spec(i)))

    def e_clear_states(self, mask=0):
        if not self.book.stores:
            return False
        return self.emit(mk("clear_states", active=self.mask() if mask == 0 else mask))

    def e_clone_state_to_phi(self, mask=0):
        b = self.book
        if not b.stores or max(b.nst) == 0:
            return False
        idx = int(self.rng.integers(max(b.nst)))
        mask = self.mask(lambda m: idx < b.nst[m]) if mask == 0 else mask
        return mask is not False and self.emit(mk("clone_state_to_phi", active=mask, idx=idx))

    def ks(self, mask, top=None):
        b = self.book
        return tuple(int(self.rng.integers(1, min(b.nst[m], top or 99) + 1)) if (mask is None or mask[m]) and b.nst[m] else 0 for m in range(self.B))

    def e_ritz_matrices(self, mask=0, ks=None):
        b = self.book
        mask = self.mask(lambda m: b.nst[m] >= 1) if mask == 0 else mask
        return mask is not False and self.emit(mk("ritz_matrices", active=mask, ks=self.ks(mask) if ks is None else ks))

    def e_rotate_states(self, mask=0):
        b = self.book
        mask = self.mask(lambda m: b.nst[m] >= 1) if mask == 0 else mask
        if mask is False:
            return False
        ks = self.ks(mask)
        return self.emit(mk("rotate_states", active=mask, coefs=tuple(("rot", self.aseed(), k) if k else None for k in ks)))

    def e_ritz(self, mask=0):
        b = self.book
        mask = self.mask(lambda m: b.nst[m] >= 1) if mask == 0 else mask
        return mask is not False and self.emit(mk("ritz", active=mask, ks=self.ks(mask)))

    def e_observables(self):
        return self.emit(mk("observables"))

    def solve_args(self):
        su = int(self.pick([1, 2, 3]))
        # loose: from a rough start the energy moves by about 1 per block at first, by a few hundredths after some tens of steps
        return dict(tolerance=float(self.pick([1.0, 0.3, 0.1, 0.03])), screen_update=su, max_steps=su * int(self.pick([3, 4, 5])))

    def e_solve(self):
        return self.emit(mk("solve", **self.solve_args()))

    def e_solve_state(self):
        b = self.book
        if not b.stores:
            return False
        wnum = int(self.rng.integers(0, min(b.nst) + 1)) if self.excited else 0
        return self.emit(mk("solve_state", wnum=wnum, **self.solve_args()))

    def e_refused(self):
        """a call the library must refuse, with the code it must give; nothing may change"""
        b = self.book
        if self.n_refused >= max(1, self.n_ops // 10) - 1:
            return False
        cands = []
        if not b.stores:
            cands += [mk("push_state", refused=WAFER_ERR_INVALID), mk("evolve", steps=2, wnum=1, refused=WAFER_ERR_INVALID),
                      mk("clone_state_to_phi", idx=0, refused=WAFER_ERR_INVALID), mk("orthogonalise", wnum=1, refused=WAFER_ERR_INVALID),
                      mk("set_gs_variant", variant=1, refused=WAFER_ERR_INVALID),
                      mk("load_state", i=0, idx=0, state=self.state_spec(0), refused=WAFER_ERR_INVALID)]
        else:
            mask = self.mask()
            act = self.members_of(mask)
            low = min(b.nst[m] for m in act)
            if low + 1 <= max(b.cap):
                cands.append(mk("evolve", active=mask, steps=int(self.pick(EVOLVE_STEPS)), wnum=low + 1, refused=WAFER_ERR_STATE))
                cands.append(mk("orthogonalise", active=mask, wnum=low + 1, refused=WAFER_ERR_STATE))
            i = int(self.rng.integers(self.B))
            cands.append(mk("load_state", i=i, idx=b.nst[i] + 1, state=self.state_spec(i), refused=WAFER_ERR_STATE))
            cands.append(mk("clone_state_to_phi", active=mask, idx=low, refused=WAFER_ERR_STATE))
            full = [m for m in range(self.B) if b.nst[m] >= b.cap[m]]
            if full:
                cands.append(mk("push_state", active=tuple(1 if m == full[0] or self.rng.random() < 0.5 else 0 for m in range(self.B)), refused=WAFER_ERR_STATE))
        op = self.pick(cands)
        assert b.why_invalid(op) is not None, op
        self.ops.append(op)
        self.n_refused += 1
        return True

    # -- motifs: short runs of ops, each aimed at one piece of kept state ----------------------------------------------------------------
    def ensure_states(self, n=1):
        """every member holds at least n states: one load, or one resample for all the members that lack state idx"""
        b = self.book
        for idx in range(n):
            short = [m for m in range(self.B) if b.nst[m] == idx]
            if len(short) == 1:
                self.e_load_state(short[0], idx)
            elif short:
                self.emit(mk("resample_state", active=None if len(short) == self.B else tuple(1 if m in short else 0 for m in range(self.B)),
                             idx=idx, src=("normal", self.aseed(), (9, 6, 5), 0.03), basis="padded"))

    def fresh_phi(self, mask=None):
        """a phi that is a copy of a stored state is replaced: one upload, or one resample for all such members"""
        stale = [m for m in self.members_of(mask) if self.book.in_store[m]]
        if len(stale) == 1:
            self.e_upload_phi(stale[0])
        elif stale:
            self.emit(mk("resample_phi", active=None if len(stale) == self.B else tuple(1 if m in stale else 0 for m in range(self.B)),
                         src=("normal", self.aseed(), (9, 6, 5), 1.0), basis="padded"))

    def m_first_onepass(self):
        """f: norm2, the first one-pass call (gs_partials regrown), norm2"""
        self.ensure_states(1)
        self.e_norm2()
        self.emit(mk("set_gs_variant", variant=1))
        self.e_excited_evolve(None)
        return self.e_norm2()

    def store_change(self, which=None):
        """one op that changes some store, and the members it changed"""
        b = self.book
        which = which or self.pick(["push", "load", "resample", "rotate", "clear_push"])
        if which == "push":
            self.fresh_phi(None)
            ok = self.e_push_state()
        elif which == "load":
            i = int(self.rng.integers(self.B))
            ok = b.nst[i] > 0 and self.e_load_state(i, int(self.rng.integers(b.nst[i])))   # an overwrite
        elif which == "resample":
            ok = self.e_resample_state()
        elif which == "rotate":
            ok = self.e_rotate_states()
        else:
            self.fresh_phi(None)
            mask = self.mask()
            self.make_unit(mask)
            ok = self.e_clear_states(mask) and self.e_push_state(mask)
        return ok and touched(self.ops[-1], self.B)

    def m_store_then_onepass(self, which=None):
        """a: a store change directly before a one-pass excited evolve or orthogonalise that reads what changed.  The Gram matrix
        holds the products of PAIRS of stored states, so the call takes wnum >= 2 and reaches the state that changed -- but after
        clear_states and one push, where a member holds one state"""
        b = self.book
        if not (self.excited and b.stores):
            return False
        which = which or self.pick(["push", "load", "resample", "rotate", "clear_push"])
        if b.gs_variant != 1:
            self.m_first_onepass() if b.gs_variant == -1 else self.emit(mk("set_gs_variant", variant=1))
        if which == "push":   # room for one more everywhere
            full = tuple(1 if b.nst[m] >= b.cap[m] else 0 for m in range(self.B))
            if any(full):
                self.emit(mk("clear_states", active=full))
        self.ensure_states(1 if which in ("push", "clear_push") else 2)
        changed = self.store_change(which)
        if not changed:
            return False
        m = self.pick(changed)
        low = 1 if which == "clear_push" else 2
        if b.nst[m] < low:
            return False
        # with m go members whose stores are at least as long, so that wnum reaches the end of m's store (up to the one-pass form's 4)
        mask = tuple(1 if x == m or (b.nst[x] >= b.nst[m] and not b.in_store[x] and self.rng.random() < 0.5) else 0 for x in range(self.B))
        wnum = min(b.nst[m], 4)
        if self.rng.random() < 0.3 and not any(b.in_store[x] for x in self.members_of(mask)):
            return self.emit(mk("orthogonalise", active=mask, wnum=wnum))
        return self.e_evolve(mask, wnum)

    def m_masked_then_all(self, nxt=None):
        """b: a masked evolve with an odd step count (or a masked symmetrise) flips some members' current buffer; then a call over all"""
        mask = self.mask(proper=True)
        if self.ext == 3 and self.rng.random() < 0.4:
            cons = tuple(self.pick(CONSTRAINTS[1:]) for _ in range(self.B))
            self.emit(mk("symmetrise", active=mask, constraints=cons))
        else:
            self.emit(mk("set_step_variant", variant=0))
            self.e_evolve(mask, 0, int(self.pick([1, 3, 5, 7])))
        nxt = nxt or self.pick(["observables", "norm2", "evolve", "ritz_matrices"])
        if nxt == "ritz_matrices" and self.book.stores:
            self.ensure_states_before_last(1)
            return self.e_ritz_matrices(None)
        if nxt == "evolve":
            return self.e_evolve(None, 0)
        return self.e_norm2() if nxt == "norm2" else self.e_observables()

    def ensure_states_before_last(self, n):
        """ensure_states, with the loads placed before the last op so that it stays directly before what follows"""
        last = self.ops.pop()
        self.ensure_states(n)
        self.ops.append(last)

    def m_active_sets(self):
        """c: evolve under A, under B != A, under A again (the kept workgroup table); then A under K = 1 and under the fused K"""
        A = self.mask(proper=True)
        Bm = self.mask(proper=True)
        if A is False or Bm is False or A == Bm:
            return False
        for msk in (A, Bm, A):
            self.e_evolve(msk, 0)
        self.emit(mk("set_step_variant", variant=0))
        self.e_evolve(A, 0, int(self.pick(EVOLVE_STEPS)))
        self.emit(mk("set_step_variant", variant=1))
        return self.e_evolve(A, 0, int(self.pick([s for s in EVOLVE_STEPS if s >= self.K])))

    def m_closed_form(self):
        """d: a closed-form V, an excited evolve, a V from the host, an excited evolve"""
        b = self.book
        if not (self.excited and b.stores):
            return False
        self.ensure_states(1)
        i = int(self.rng.integers(self.B))
        self.emit(mk("set_potential", i=i, pot=self.pick(CLOSED_FORM)))
        mask = tuple(1 if m == i or self.rng.random() < 0.5 else 0 for m in range(self.B))
        self.e_excited_evolve(mask)
        if self.rng.random() < 0.5:
            self.e_set_potential_host(i)
        else:
            self.e_resample_potential(tuple(1 if m == i else 0 for m in range(self.B)))
        return self.e_excited_evolve(mask)

    def m_potsub(self, nxt=None):
        """e: a pot_sub kind change directly before observables, or before ritz_matrices"""
        i = int(self.rng.integers(self.B))
        nxt = nxt or self.pick(["observables", "ritz_matrices"])
        if self.book.stores and nxt == "ritz_matrices":
            self.ensure_states(1)
            self.e_set_potsub(i, int(self.rng.integers(3)))
            self.e_set_potsub(i, (self.ops[-1]["kind"] + 1 + int(self.rng.integers(2))) % 3)
            return self.e_ritz_matrices(None)
        self.e_set_potsub(i, int(self.rng.integers(3)))
        self.e_set_potsub(i, (self.ops[-1]["kind"] + 1 + int(self.rng.integers(2))) % 3)
        return self.e_observables()

    def m_empty_stores(self):
        """g: every store emptied (the slots are freed), filled again, an excited evolve, ritz"""
        b = self.book
        if not (self.excited and b.stores):
            return False
        self.ensure_states(1)
        self.emit(mk("clear_states"))
        self.fresh_phi(None)
        if self.rng.random() < 0.5:
            self.e_push_state(None)
        else:
            self.ensure_states(1)
        self.fresh_phi(None)
        self.e_excited_evolve(None)
        return self.e_ritz(None)

    def m_write_then_fused(self, which=None):
        """h: phi written by another call directly before a fused pass"""
        b = self.book
        self.emit(mk("set_step_variant", variant=1))
        which = which or self.pick(list(PHI_WRITERS))
        if which == "clone_state_to_phi" and b.stores:
            self.ensure_states(1)
        if which == "symmetrise" and self.ext == 3:
            mask = self.mask()
            self.emit(mk("symmetrise", active=mask, constraints=tuple(self.pick(CONSTRAINTS[1:]) for _ in range(self.B))))
        elif which == "clone_state_to_phi" and b.stores and max(b.nst) > 0:
            self.e_clone_state_to_phi()
            mask = self.ops[-1].active
        elif which == "upload_phi":
            self.e_upload_phi()
            mask = tuple(1 if m == self.ops[-1]["i"] or self.rng.random() < 0.5 else 0 for m in range(self.B))
        else:
            if not self.e_resample_phi():
                return False
            mask = self.ops[-1].active
        return self.e_evolve(mask, 0, int(self.pick([s for s in EVOLVE_STEPS if s >= self.K])))

    def m_ritz_grows(self):
        """i: a ritz* call, stores that grow, a call with a larger k"""
        b = self.book
        if not b.stores or min(b.cap) < 2:
            return False
        self.ensure_states(1)
        k = min(b.nst)
        if any(b.nst[m] >= b.cap[m] for m in range(self.B)):
            self.emit(mk("clear_states"))
            self.ensure_states(1)
            k = 1
        self.e_ritz_matrices(None, tuple([k] * self.B))
        self.fresh_phi(None)
        if self.rng.random() < 0.5:
            self.e_push_state(None)
        else:
            self.ensure_states(k + 1)
        call = self.pick(["ritz_matrices", "ritz"])
        return self.emit(mk(call, ks=tuple([k + 1] * self.B)))

    def m_solve(self):
        """j: a solve whose members stop at different blocks, then an evolve of all"""
        self.emit(mk("resample_phi", src=("normal", self.aseed(), (9, 6, 5), 1.0), basis="padded"))   # a rough start for everyone
        su = int(self.pick([1, 2, 3]))
        if not self.emit(mk("solve", tolerance=float(self.pick([1.0, 0.5])), screen_update=su, max_steps=su * int(self.pick([4, 5, 6])))):
            return False
        return self.e_evolve(None, 0)

    def m_wnum5(self):
        """wnum 5 under the one-pass variant: the sequential fallback"""
        b = self.book
        if not (self.excited and b.stores and min(b.cap) >= 5):
            return False
        if b.gs_variant != 1:
            self.m_first_onepass() if b.gs_variant == -1 else self.emit(mk("set_gs_variant", variant=1))
        self.ensure_states(5)
        self.fresh_phi(None)
        return self.e_evolve(None, 5, int(self.pick([1, 2, 3])))

    # -- the program -------------------------------------------------------------------------------------------------------------------------
    def prologue(self):
        """every member gets a potential and a start, in one launch each or member by member"""
        if self.rng.random() < 0.6:
            self.e_set_potentials(None)
        else:
            for m in range(self.B):
                if self.rng.random() < 0.5:
                    self.emit(mk("set_potential", i=m, pot=self.pick(ALGEBRAIC)))
                else:
                    self.e_set_potential_host(m)
        if self.rng.random() < 0.6:
            self.e_set_initial_conditions(None)
        else:
            for m in range(self.B):
                if self.rng.random() < 0.5:
                    self.emit(mk("set_initial_condition", i=m, ic=self.pick(ICS), seed=int(self.rng.integers(100))))
                else:
                    self.e_upload_phi(m)

    def agenda(self):
        """the motifs this program must hold, so that the seed list of a kind reaches every transition whatever the dice say: each
        variant goes to one seed of the kind (the excited ones to one of the seeds with excited-state calls), symmetrise to ext 3"""
        b, s = self.book, self.seed
        ground = [(self.m_masked_then_all, "observables"), (self.m_masked_then_all, "norm2"), (self.m_masked_then_all, "evolve"),
                  (self.m_active_sets,), (self.m_potsub, "observables"), (self.m_write_then_fused, "upload_phi"),
                  (self.m_write_then_fused, "resample_phi"), (self.m_solve,)]
        stores = [(self.m_masked_then_all, "ritz_matrices"), (self.m_potsub, "ritz_matrices"), (self.m_write_then_fused, "clone_state_to_phi"),
                  (self.m_ritz_grows,)]
        excited = [(self.m_store_then_onepass, w) for w in ("push", "clear_push", "load", "resample", "rotate")] + [
            (self.m_closed_form,), (self.m_empty_stores,)]
        out = [v for k, v in enumerate(ground) if k % 6 == s % 6]
        if b.stores:
            out += [v for k, v in enumerate(stores) if (k + 1) % 6 == s % 6 or (k + 4) % 6 == s % 6]
        if self.excited and b.stores:
            rank = [x for x in range(6) if not ground_only(x, self.kind)].index(s % 6)
            out += [v for k, v in enumerate(excited) if k % 4 == rank]
            if min(b.cap) >= 5:
                out.append((self.m_wnum5,))
        if self.ext == 3:
            out += [(self.m_write_then_fused, "symmetrise"), (self.e_symmetrise,), (self.e_symmetrise,)]
        return out

    def musts(self):
        """the single ops this program must hold at least once: every other op kind by the seed's parity, and those that only some
        programs can hold (excited-state calls) in each of them -- every kind then occurs three times over six seeds"""
        names = {"set_potential": self.e_set_potential, "set_potentials": self.e_set_potentials, "set_potential_host": self.e_set_potential_host,
                 "set_potsub": self.e_set_potsub, "set_initial_condition": self.e_set_initial_condition,
                 "set_initial_conditions": self.e_set_initial_conditions, "upload_phi": self.e_upload_phi, "resample_phi": self.e_resample_phi,
                 "resample_potential": self.e_resample_potential, "resample_potsub": self.e_resample_potsub, "resample_state": self.e_resample_state,
                 "evolve": self.e_evolve, "set_step_variant": self.e_set_step_variant, "set_gs_variant": self.e_set_gs_variant, "norm2": self.e_norm2,
                 "normalise": self.e_normalise, "orthogonalise": self.e_orthogonalise, "push_state": self.e_push_state,
                 "load_state": self.e_load_state, "clear_states": self.e_clear_states, "clone_state_to_phi": self.e_clone_state_to_phi,
                 "ritz_matrices": self.e_ritz_matrices, "rotate_states": self.e_rotate_states, "ritz": self.e_ritz,
                 "observables": self.e_observables, "solve": self.e_solve, "refused": self.e_refused}
        return [(name, fn) for k, (name, fn) in enumerate(names.items()) if k % 2 == self.seed % 2 or name == "orthogonalise"]

    def run(self):
        self.prologue()
        singles = [
            (self.e_set_potential, 2), (self.e_set_potentials, 2), (self.e_set_potential_host, 2), (self.e_set_potsub, 3),
            (self.e_set_initial_condition, 2), (self.e_set_initial_conditions, 2), (self.e_upload_phi, 3),
            (self.e_resample_phi, 3), (self.e_resample_potential, 3), (self.e_resample_potsub, 3), (self.e_resample_state, 3),
            (self.e_symmetrise, 5), (self.e_evolve, 8), (self.e_excited_evolve, 6), (self.e_set_step_variant, 3), (self.e_set_gs_variant, 3),
            (self.e_norm2, 3), (self.e_normalise, 3), (self.e_orthogonalise, 3), (self.e_push_state, 4), (self.e_load_state, 4),
            (self.e_clear_states, 1), (self.e_clone_state_to_phi, 2), (self.e_ritz_matrices, 3), (self.e_rotate_states, 4), (self.e_ritz, 2),
            (self.e_observables, 3), (self.e_solve, 2), (self.e_refused, 4),
        ]
        w = np.array([x[1] for x in singles], dtype=float)
        w /= w.sum()

        def single():
            return singles[int(self.rng.choice(len(singles), p=w))][0]()

        tasks = [("motif", v) for v in self.agenda()] + [("must", v) for v in self.musts()]
        for k in self.rng.permutation(len(tasks)):
            what, v = tasks[int(k)]
            if what == "motif":
                v[0](*v[1:])
            elif not any(op.name == v[0] and op.refused is None for op in self.ops) and not (v[0] == "refused" and self.n_refused):
                for _ in range(20):
                    if v[1]():
                        break
            if self.rng.random() < 0.4:
                single()
        guard = 0
        while len(self.ops) < self.n_ops and guard < 100 * self.n_ops:
            guard += 1
            single()
        if self.book.stores:   # last: which members solve_state pushes only a run tells, so no later op may depend on it
            full = tuple(1 if self.book.nst[m] >= self.book.cap[m] else 0 for m in range(self.B))
            if any(full):
                self.emit(mk("clear_states", active=full))
            self.fresh_phi(None)
            self.e_solve_state()
        return self.ops


def program(seed, kind, ext, dtype="f64", n_ops=N_OPS):
    """the ops of one program: a pure function of its arguments (the dtype does not enter: one program serves all three)"""
    assert kind in KINDS and ext in (1, 2, 3) and dtype in DTYPES
    return list(_Gen(seed, kind, ext, n_ops).run())


def check_valid(prog, mems, kind, ext):
    """replay the generator's bookkeeping over a program: every op is valid, or refused on purpose and invalid"""
    book = Book(mems, kind, ext)
    for idx, op in enumerate(prog):
        why = book.why_invalid(op)
        if op.refused is not None:
            assert why is not None, "op %d %r is marked refused but is valid" % (idx, op)
        else:
            assert why is None, "op %d %r is invalid: %s" % (idx, op, why)
            book.commit(op)
            assert op.name != "solve_state" or idx == len(prog) - 1, "solve_state's pushes are not book-kept: it must be the last op"
    return book


# ---- one call on a Batch ---------------------------------------------------------------------------------------------------------------
class Env:
    """what an executor remembers between calls: the norms the last norm2 read"""

    def __init__(self, n):
        self.norm2 = [None] * n


def call_batch(b, op, env):
    """make the call on the Batch b -> its return value as one entry per member (None where the call returns nothing)"""
    n = op.name
    B = len(b)
    a = None if op.active is None else list(op.active)
    out = [None] * B
    if n == "set_potential":
        b.set_potential(op["i"], op["pot"])
    elif n == "set_potentials":
        b.set_potentials(list(op["names"]), active=a)
    elif n == "set_potential_host":
        b.set_potential_host(op["i"], materialise(op["v"]), op["potsub_kind"], op["potsub_scalar"], materialise(op["potsub"]))
    elif n == "set_potsub":
        b.set_potsub(op["i"], op["kind"], op["scalar"], materialise(op["potsub"]))
    elif n == "set_initial_condition":
        b.set_initial_condition(op["i"], op["ic"], seed=op["seed"])
    elif n == "set_initial_conditions":
        b.set_initial_conditions(list(op["names"]), seeds=list(op["seeds"]), active=a)
    elif n == "upload_phi":
        b.upload_phi(op["i"], materialise(op["phi"]))
    elif n in ("resample_phi", "resample_potential", "resample_potsub"):
        src = op["src"]
        getattr(b, n)(src if isinstance(src, tuple) and src[0] in ("member", "state") else materialise(src), active=a, basis=op["basis"])
    elif n == "resample_state":
        src = op["src"]
        b.resample_state(op["idx"], src if isinstance(src, tuple) and src[0] in ("member", "state") else materialise(src), active=a, basis=op["basis"])
    elif n == "symmetrise":
        b.symmetrise(list(op["constraints"]), active=a)
    elif n == "evolve":
        b.evolve(op["steps"], active=a, wnum=op["wnum"])
    elif n == "set_step_variant":
        b.set_step_variant(op["variant"])
    elif n == "set_gs_variant":
        b.set_gs_variant(op["variant"])
    elif n == "norm2":
        out = b.norm2()
        env.norm2 = list(out)
    elif n == "normalise":
        b.normalise([1.0 if x is None else x for x in env.norm2], active=a)
    elif n == "orthogonalise":
        b.orthogonalise(op["wnum"], active=a)
    elif n == "push_state":
        b.push_state(active=a)
    elif n == "load_state":
        b.load_state(op["i"], op["idx"], materialise(op["state"]))
    elif n == "clear_states":
        b.clear_states(active=a)
    elif n == "clone_state_to_phi":
        b.clone_state_to_phi(op["idx"], active=a)
    elif n == "ritz_matrices":
        out = b.ritz_matrices(list(op["ks"]), active=a)
    elif n == "rotate_states":
        b.rotate_states([materialise(c) for c in op["coefs"]], active=a)
    elif n == "ritz":
        out = [None if r is None else norm_ritz(r) for r in b.ritz(list(op["ks"]), active=a)]
    elif n == "observables":
        out = b.observables()
    elif n == "solve":
        out = [r[:3] for r in b.solve(op["tolerance"], op["screen_update"], op["max_steps"])]
    elif n == "solve_state":
        out = [r[:3] for r in b.solve_state(op["wnum"], op["tolerance"], op["screen_update"], op["max_steps"])]
    else:
        raise ValueError("unknown op %r" % (op,))
    return out


def norm_ritz(r):
    """a ritz result in one form for Batch and Context: a failed solve is its status alone"""
    if r.get("status", WAFER_OK) != WAFER_OK:
        return {"status": r["status"]}
    return {"status": WAFER_OK, "evals": r["evals"], "coef": r["coef"], "h": r["h"], "s": r["s"]}


def snapshot_batch(b, m, book):
    """member m's whole state as the batch holds it"""
    nst = b.num_states()[m]
    kind, scalar = b.potsub(m)
    return {"phi": b.download_phi(m) if book.have_phi[m] else None,
            "v": b.download_array(m, "v") if book.have_pot[m] else None,
            "potsub": (kind, scalar),
            "potsub_arr": b.download_array(m, "potsub") if kind == 2 else None,
            "nst": nst,
            "states": [b.download_state(m, l) for l in range(nst)] if book.stores else []}


def make_batch(wa, mems, kind, ext, dtype):
    pars = [params_of(wa, mem, ext, dtype) for mem in mems]
    if kind == "one_shape":
        return wa.Batch(pars)
    return wa.Batch(pars, mixed_shapes=True, state_stores=(kind == "mixed_states"))


def work_cells(a, ext):
    return np.ascontiguousarray(a[ext:-ext, ext:-ext, ext:-ext])


def resolve_source(op, snaps, ext):
    """the numpy array behind a ("member", j) / ("state", j, l) source: those work cells as the snapshots hold them"""
    src = op.get("src")
    if not (isinstance(src, tuple) and src[0] in ("member", "state")):
        return None
    return work_cells(snaps[src[1]]["phi"] if src[0] == "member" else snaps[src[1]]["states"][src[2]], ext)


def project(op, m, B, src=None):
    """the op as member m alone sees it in a batch of one: None if it does not concern m (or is refused), indices and lists
    shrunk to one entry, a member source replaced by its array"""
    if op.refused is not None or m not in touched(op, B):
        return None
    kw = dict(op.kw)
    if "i" in kw:
        kw["i"] = 0
    for key in ("names", "seeds", "constraints", "ks", "coefs"):
        if key in kw:
            kw[key] = (kw[key][m],)
    if src is not None:
        kw["src"] = src
    return Op(op.name, tuple(kw.items()), None if op.active is None else (1,), None)


# ---- comparing, and saying what differs ----------------------------------------------------------------------------------------------------
class SequenceFailure(AssertionError):
    pass


def first_difference(got, want, bits=True):
    """None if the two values hold the same bytes, else a description of the first place where they do not; values: None, numbers,
    arrays, and tuples, lists and dicts of them.  bits=False: equal values instead, as np.array_equal(equal_nan=True) has them
    (0.0 and -0.0 are equal)"""
    if got is None or want is None:
        return None if got is None and want is None else "%r against %r" % (type(got).__name__, type(want).__name__)
    if isinstance(got, dict):
        if sorted(got) != sorted(want):
            return "keys %s against %s" % (sorted(got), sorted(want))
        for k in sorted(got):
            d = first_difference(got[k], want[k], bits)
            if d:
                return "[%r] %s" % (k, d)
        return None
    if isinstance(got, (tuple, list)):
        if len(got) != len(want):
            return "length %d against %d" % (len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            d = first_difference(g, w, bits)
            if d:
                return "[%d] %s" % (k, d)
        return None
    if isinstance(got, np.ndarray):
        if got.shape != want.shape:
            return "shape %s against %s" % (got.shape, want.shape)
        g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
        if bits:
            bad = np.flatnonzero(g.view(np.uint64).ravel() != w.view(np.uint64).ravel())
        else:
            bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))).ravel())
        if bad.size == 0:
            return None
        cell = np.unravel_index(int(bad[0]), g.shape)
        return "%d of %d cells differ, the first at %s: %r against %r" % (bad.size, g.size, tuple(int(c) for c in cell), float(g[cell]), float(w[cell]))
    if isinstance(got, float) or isinstance(want, float):
        if not bits:
            return None if _close(got, want) else "%r against %r" % (got, want)
        return None if struct.pack("d", float(got)) == struct.pack("d", float(want)) else "%r against %r" % (got, want)
    return None if got == want else "%r against %r" % (got, want)


def compare_exact(got, want):
    """the first difference between two snapshots or return values, as 'what: where'"""
    if isinstance(got, dict) and "phi" in got and "states" in got:
        for key in ("nst", "potsub", "phi", "v", "potsub_arr"):
            d = first_difference(got[key], want[key])
            if d:
                return "%s: %s" % (key, d)
        for l, (g, w) in enumerate(zip(got["states"], want["states"])):
            d = first_difference(g, w)
            if d:
                return "stored state %d: %s" % (l, d)
        return None
    d = first_difference(got, want)
    return "return value: " + d if d else None


def describe(case, prog, idx, member, tier, what):
    seed, kind, ext, dtype = case
    lines = ["%s: seed %d, kind %s, ext %d, dtype %s: op %d %r, member %s: %s" % (tier, seed, kind, ext, dtype, idx, prog[idx], member, what),
             "replay: python -m tests.batch_sequences --seed %d --kind %s --ext %d" % (seed, kind, ext), "the program up to that op:"]
    lines += ["  %3d  %r" % (k, op) for k, op in enumerate(prog[:idx + 1])]
    return "\n".join(lines)


# ---- T1 and T2: the executors ----------------------------------------------------------------------------------------------------------
def run_batch(wa, prog, mems, kind, ext, dtype, on_op=None):
    """the program on the batch under test -> per op (snapshots of every member, return values per member).  on_op(idx, op, before,
    after, ret) is called after every op with the snapshots around it.  A refused op must raise its code and change nothing."""
    B = len(mems)
    book, env, trace = Book(mems, kind, ext), Env(B), []
    with make_batch(wa, mems, kind, ext, dtype) as b:
        before = [snapshot_batch(b, m, book) for m in range(B)]
        for idx, op in enumerate(prog):
            ret = [None] * B
            if op.refused is not None:
                try:
                    call_batch(b, op, Env(B))
                except wa.WaferError as e:
                    if e.code != op.refused:
                        raise SequenceFailure("op %d %r: refused with code %d, not %d (%s)" % (idx, op, e.code, op.refused, e))
                else:
                    raise SequenceFailure("op %d %r was not refused" % (idx, op))
            else:
                ret = call_batch(b, op, env)
                book.commit(op)
            after = [snapshot_batch(b, m, book) for m in range(B)]
            for m in range(B):   # inactive members and the members of refused calls keep every byte
                if op.refused is not None or m not in touched(op, B):
                    d = compare_exact(after[m], before[m])
                    if d:
                        raise SequenceFailure("op %d %r: member %d is not concerned and changed: %s" % (idx, op, m, d))
            trace.append((after, ret))
            if on_op:
                on_op(idx, op, before, after, ret)
            before = after
    return trace


class Solo:
    """member m alone in a plain Batch([par_m]), fed the projection of the program onto m"""

    def __init__(self, wa, mems, m, ext, dtype):
        self.B, self.m, self.ext = len(mems), m, ext
        self.book, self.env = Book([mems[m]], "one_shape", ext), Env(1)
        self.b = wa.Batch([params_of(wa, mems[m], ext, dtype)])

    def step(self, op, src):
        """-> (snapshot, return value) after the op, or None where it does not concern the member"""
        op1 = project(op, self.m, self.B, src)
        if op1 is None:
            return None
        ret = call_batch(self.b, op1, self.env)
        self.book.commit(op1)
        return snapshot_batch(self.b, 0, self.book), ret[0]

    def close(self):
        self.b.close()


def run_solo(wa, prog, mems, m, ext, dtype, sources):
    """member m alone -> per op (snapshot, return value) or None; sources[idx]: the array behind op idx's member source"""
    solo = Solo(wa, mems, m, ext, dtype)
    try:
        return [solo.step(op, sources[idx]) for idx, op in enumerate(prog)]
    finally:
        solo.close()


class FreeContext:
    """member m as a free-running Context of its Params (ground-only programs)"""

    def __init__(self, wa, mems, m, ext, dtype):
        self.wa, self.B, self.m, self.ext = wa, len(mems), m, ext
        self.par = params_of(wa, mems[m], ext, dtype)
        self.c = wa.Context(self.par)
        self.book, self.norm2 = Book([mems[m]], "one_shape", ext), None

    def step(self, op, src):
        op1 = project(op, self.m, self.B, src)
        if op1 is None:
            return None
        ret = self.call(op1)
        self.book.commit(op1)
        return self.snapshot(), ret

    def call(self, op):
        c, n = self.c, op.name
        basis = None if op.get("basis") == "padded" else self.par.work_shape
        if n in ("set_potential", "set_potentials"):
            c.set_potential(op["pot"] if n == "set_potential" else op["names"][0])
        elif n == "set_potential_host":
            c.set_potential_host(materialise(op["v"]), op["potsub_kind"], op["potsub_scalar"], materialise(op["potsub"]))
        elif n == "set_potsub":
            c.set_potsub(op["kind"], op["scalar"], materialise(op["potsub"]))
        elif n in ("set_initial_condition", "set_initial_conditions"):
            c.set_initial_condition(*((op["ic"], op["seed"]) if n == "set_initial_condition" else (op["names"][0], op["seeds"][0])))
        elif n == "upload_phi":
            c.upload_phi(materialise(op["phi"]))
        elif n == "resample_phi":
            c.upload_phi_resampled(materialise(op["src"]), basis=basis)
        elif n == "resample_potential":
            c.set_potential_resampled(materialise(op["src"]), basis=basis)
        elif n == "resample_potsub":
            c.set_potsub_resampled(materialise(op["src"]))
        elif n == "resample_state":   # a Context has no such call: resample into phi, load that as the state, put phi back
            keep = c.download_phi() if self.book.have_phi[0] else None
            c.upload_phi_resampled(materialise(op["src"]), basis=basis)
            c.load_state(op["idx"], c.download_phi())
            if keep is not None:
                c.upload_phi(keep)
        elif n == "symmetrise":
            c.symmetrise(op["constraints"][0])
        elif n == "evolve":
            assert op["wnum"] == 0, "run_contexts takes ground-only programs"
            c.evolve(0, op["steps"])
        elif n in ("set_step_variant", "set_gs_variant"):
            pass   # a Batch's dispatch: the bits are promised to be the same
        elif n == "norm2":
            self.norm2 = c.norm2()
            return self.norm2
        elif n == "normalise":
            c.normalise(1.0 if self.norm2 is None else self.norm2)
        elif n == "push_state":
            c.push_state()
        elif n == "load_state":
            c.load_state(op["idx"], materialise(op["state"]))
        elif n == "clear_states":
            c.clear_states()
        elif n == "clone_state_to_phi":
            c.clone_state_to_phi(op["idx"])
        elif n == "ritz_matrices":
            return c.ritz_matrices(op["ks"][0])
        elif n == "rotate_states":
            c.rotate_states(materialise(op["coefs"][0]))
        elif n == "ritz":
            try:
                return norm_ritz(c.ritz(op["ks"][0]))
            except self.wa.WaferError as e:
                return {"status": e.code}
        elif n == "observables":
            return c.observables()
        elif n in ("solve", "solve_state"):
            assert op.get("wnum", 0) == 0, "run_contexts takes ground-only programs"
            out = c.solve_state(0, op["tolerance"], op["screen_update"], op["max_steps"])
            if n == "solve" and out[2]:   # a Context pushes what converged, Batch.solve pushes nothing: take the state off again
                keep = [c.download_state(l) for l in range(c.num_states() - 1)]
                c.clear_states()
                for l, s in enumerate(keep):
                    c.load_state(l, s)
            return out
        else:
            raise ValueError("no Context form of %r" % (op,))
        return None

    def snapshot(self):
        c = self.c
        nst = c.num_states()
        kind, scalar = c.potsub()
        return {"phi": c.download_phi() if self.book.have_phi[0] else None, "v": c.download_array("v") if self.book.have_pot[0] else None,
                "potsub": (kind, scalar), "potsub_arr": c.download_array("potsub") if kind == 2 else None, "nst": nst,
                "states": [c.download_state(l) for l in range(nst)]}

    def close(self):
        self.c.close()


def run_contexts(wa, prog, mems, ext, dtype, sources):
    """one free-running Context per member -> per member, per op (snapshot, return value) or None"""
    out = []
    for m in range(len(mems)):
        fc = FreeContext(wa, mems, m, ext, dtype)
        try:
            out.append([fc.step(op, sources[idx]) for idx, op in enumerate(prog)])
        finally:
            fc.close()
    return out


# ---- T3: one member on the CPU ---------------------------------------------------------------------------------------------------------
class HostModel:
    """one member's (phi, V, pot_sub kind / scalar / array, states) on the CPU, fp64, from oracle.wafer_oracle and tests/ritz_model
    and nothing else.  apply(op) takes a projected op (project()); load(snapshot) sets the state to what a device held."""

    def __init__(self, wo, mem, ext):
        self.wo, self.mem, self.ext = wo, mem, ext
        self.phi = self.v = None
        self.potsub = (0, 0.0, None)
        self.states = []
        self.norm2 = None

    def cfg(self, potential="Harmonic"):
        return config_of(self.wo, self.mem, self.ext, potential)

    def load(self, snap):
        cp = lambda a: None if a is None else np.array(a, dtype=np.float64, order="C")  # noqa: E731
        self.phi, self.v = cp(snap["phi"]), cp(snap["v"])
        self.potsub = (snap["potsub"][0], snap["potsub"][1], cp(snap["potsub_arr"]))
        self.states = [cp(s) for s in snap["states"]]

    def snapshot(self):
        return {"phi": None if self.phi is None else self.phi.copy(), "v": None if self.v is None else self.v.copy(),
                "potsub": self.potsub[:2], "potsub_arr": self.potsub[2].copy() if self.potsub[0] == 2 else None,
                "nst": len(self.states), "states": [s.copy() for s in self.states]}

    def framed(self, work):
        e = self.ext
        out = np.zeros(padded(self.mem.shape, e))
        out[e:-e, e:-e, e:-e] = work
        return out

    def resampled(self, src, basis):
        shape = self.mem.shape
        return self.wo.trilerp_resize(materialise(src), shape, basis=padded(shape, self.ext) if basis == "padded" else shape)

    def ab(self):
        return self.wo.ab(self.cfg(), self.v)

    def apply(self, op, device=None):
        """the op on the model -> its return value.  device: the device's return value of the same call, from which a ritz takes the
        coefficients (its host solve is tests/test_ritz_host.py's subject) so that the rotation is compared on the same matrix"""
        wo, n, cfg = self.wo, op.name, self.cfg()
        if n in ("set_potential", "set_potentials"):
            c = self.cfg(op["pot"] if n == "set_potential" else op["names"][0])
            self.v, self.potsub = wo.potential_generate(c), wo.potential_sub(c)
        elif n == "set_potential_host":
            k = op["potsub_kind"]
            self.v = materialise(op["v"]).copy()
            self.potsub = (k, op["potsub_scalar"] if k == 1 else 0.0, materialise(op["potsub"]) if k == 2 else None)
        elif n == "set_potsub":
            k = op["kind"]
            self.potsub = (k, op["scalar"] if k == 1 else 0.0, materialise(op["potsub"]) if k == 2 else self.potsub[2])
        elif n in ("set_initial_condition", "set_initial_conditions"):
            ic, seed = (op["ic"], op["seed"]) if n == "set_initial_condition" else (op["names"][0], op["seeds"][0])
            self.phi = wo.initial_condition(cfg, ic, seed)
        elif n == "upload_phi":
            self.phi = materialise(op["phi"]).copy()
        elif n == "resample_phi":
            self.phi = self.framed(self.resampled(op["src"], op["basis"]))
        elif n == "resample_potential":   # potential.rs:357-358: a potential from a file has no pot_sub of its own
            self.v, self.potsub = self.framed(self.resampled(op["src"], op["basis"])), (0, 0.0, self.potsub[2])
        elif n == "resample_potsub":
            self.potsub = (2, 0.0, self.resampled(op["src"], "work"))
        elif n == "resample_state":
            self.set_state(op["idx"], self.framed(self.resampled(op["src"], op["basis"])))
        elif n == "symmetrise":
            wo.symmetrise(cfg, op["constraints"][0], self.phi)
        elif n == "evolve":
            a, b = self.ab()
            assert op["wnum"] <= len(self.states)
            wo.evolve(cfg, op["wnum"], a, b, self.phi, self.states[:op["wnum"]], max(1, op["steps"]))
        elif n in ("set_step_variant", "set_gs_variant"):
            pass
        elif n == "norm2":
            self.norm2 = wo.norm2(cfg, self.phi)
            return self.norm2
        elif n == "normalise":
            wo.normalise(self.phi, 1.0 if self.norm2 is None else self.norm2)
        elif n == "orthogonalise":
            assert op["wnum"] <= len(self.states)
            wo.orthogonalise(op["wnum"], self.phi, self.states[:op["wnum"]])
        elif n == "push_state":
            assert len(self.states) < self.mem.max_states
            self.states.append(self.phi.copy())
        elif n == "load_state":
            self.set_state(op["idx"], materialise(op["state"]).copy())
        elif n == "clear_states":
            self.states = []
        elif n == "clone_state_to_phi":
            self.phi = self.states[op["idx"]].copy()
        elif n == "ritz_matrices":
            return self.matrices(op["ks"][0])   # (h, s, sum |h terms|, sum |s terms|): the last two scale the tolerance
        elif n == "rotate_states":
            coef = materialise(op["coefs"][0])
            self.rotate(coef)
        elif n == "ritz":
            k = op["ks"][0]
            h, s, ah, as_ = self.matrices(k)
            if device is not None:
                if device["status"] != WAFER_OK:
                    return {"status": device["status"]}
                evals, coef = device["evals"], device["coef"]
            else:
                try:
                    evals, coef = ritz_solve(h, s)
                except np.linalg.LinAlgError:
                    return {"status": WAFER_ERR_STATE}
            self.rotate(coef)
            return {"status": WAFER_OK, "evals": evals, "coef": coef, "h": h, "s": s, "ah": ah, "as": as_}
        elif n == "observables":
            return wo.observables(cfg, self.v, self.phi, self.potsub if self.potsub[0] == 2 else (self.potsub[0], self.potsub[1], None))
        elif n in ("solve", "solve_state"):
            wnum = op.get("wnum", 0)
            a, b = self.ab()
            sub = self.potsub if self.potsub[0] == 2 else (self.potsub[0], self.potsub[1], None)
            rows, conv = wo.solve(cfg, wnum, self.v, a, b, self.phi, self.states[:wnum], op["tolerance"], op["screen_update"],
                                  max_steps=op["max_steps"], potsub=sub)
            if n == "solve_state" and conv:
                self.states.append(self.phi.copy())
            return rows, None, conv
        else:
            raise ValueError("unknown op %r" % (op,))
        return None

    def set_state(self, idx, state):
        assert idx <= len(self.states) and idx < self.mem.max_states
        if idx == len(self.states):
            self.states.append(state)
        else:
            self.states[idx] = state

    def matrices(self, k):
        from tests import ritz_model
        assert 1 <= k <= len(self.states)
        return ritz_model.matrices(self.cfg(), self.v, self.states[:k], scales=True)

    def rotate(self, coef):
        from tests import ritz_model
        k = len(coef)
        assert 1 <= k <= len(self.states)
        self.states[:k] = ritz_model.rotate(self.states[:k], coef)


def ritz_solve(h, s):
    """the generalised symmetric eigenproblem h c = e s c by Cholesky reduction (numpy): evals ascending, c^T s c = 1"""
    L = np.linalg.cholesky(0.5 * (s + s.T))
    Li = np.linalg.inv(L)
    evals, y = np.linalg.eigh(Li @ (0.5 * (h + h.T)) @ Li.T)
    return evals, Li.T @ y


def run_model(wo, prog, mems, ext):
    """the whole program on one free-running HostModel per member (CPU only) -> per op (snapshots, return values per member)"""
    B = len(mems)
    models = [HostModel(wo, mem, ext) for mem in mems]
    trace = []
    snaps = [mod.snapshot() for mod in models]
    for op in prog:
        src = resolve_source(op, snaps, ext)
        ret = [None] * B
        for m in range(B):
            op1 = project(op, m, B, src)
            if op1 is not None:
                ret[m] = models[m].apply(op1)
        snaps = [mod.snapshot() for mod in models]
        trace.append((snaps, ret))
    return trace


# ---- T3's bars: each op held to the bar the suite already has for it ---------------------------------------------------------------------
ATOL_EXCITED = 1e-13        # tests/test_gpu_batch_states.py: check_against_oracle(atol=1e-13), per cell after an excited evolve
ATOL_ORTHOGONALISE = 1e-14  # tests/test_gpu_batch_states.py: test_batch_orthogonalise_and_norm2_match_contexts, np.allclose(rtol=0, atol=1e-14)
GAUSSIAN_BAR = dict(rtol=1e-12, atol=1e-13)   # tests/test_gpu_parity.py: test_initial_conditions
REL_RITZ = 1e-12            # tests/test_gpu_ritz.py: test_matrices_against_the_model, relative to sum |term|
SOLVE_E_ABS, SOLVE_R_REL = 2e-9, 1e-7   # tests/test_gpu_parity.py: test_solve_matches_oracle (rows: step and tau equal, at most one row more or fewer)


def _close(got, want, rel=0.0, abs_=0.0):
    got, want = float(got), float(want)
    return got == want or (np.isnan(got) and np.isnan(want)) or abs(got - want) <= max(abs_, rel * abs(want))


def _matrix_bar(name, got, want, scale):
    bad = np.abs(got - want) > REL_RITZ * scale
    if np.any(bad):
        j = tuple(int(x) for x in np.argwhere(bad)[0])
        return "%s%s: %r against the model's %r (sum |term| %r)" % (name, j, float(got[j]), float(want[j]), float(scale[j]))
    return None


def compare_oracle(op, got, want, got_ret, want_ret, rel_sum):
    """T3: the device's snapshot and return value after op (a projected op) against the model's, which started from the device's state
    before it.  Every array np.array_equal, but for the ops whose bar in the suite is a tolerance."""
    n = op.name
    solve = n in ("solve", "solve_state")
    for key in ("nst", "potsub", "phi", "v", "potsub_arr"):
        if solve and key in ("nst", "phi"):
            continue   # the suite holds a solve's rows to the oracle, its phi to a Context (T2) and to the member alone (T1)
        g, w = got[key], want[key]
        bar = None
        if key == "phi" and n == "evolve" and op["wnum"]:
            bar = dict(rtol=0, atol=ATOL_EXCITED)
        elif key == "phi" and n == "orthogonalise":
            bar = dict(rtol=0, atol=ATOL_ORTHOGONALISE)
        elif key == "phi" and n in ("set_initial_condition", "set_initial_conditions") and "Gaussian" in (op.get("ic"), (op.get("names") or (None,))[0]):
            bar = GAUSSIAN_BAR
        if bar is None:
            d = first_difference(g, w, bits=False)   # np.array_equal, as the suite's tests of these ops compare
        else:
            d = None if np.allclose(g, w, equal_nan=True, **bar) else "max |difference| %r is above %r" % (float(np.nanmax(np.abs(g - w))), bar)
        if d:
            return "%s: %s" % (key, d)
    if not solve:
        for l, (g, w) in enumerate(zip(got["states"], want["states"])):
            d = first_difference(g, w, bits=False)
            if d:
                return "stored state %d: %s" % (l, d)
    if n == "norm2":
        return None if _close(got_ret, want_ret, rel=rel_sum) else "norm2: %r against %r" % (got_ret, want_ret)
    if n == "observables":
        for q in want_ret:
            if not _close(got_ret[q], want_ret[q], rel=rel_sum):
                return "observables[%r]: %r against %r" % (q, got_ret[q], want_ret[q])
    if n == "ritz_matrices":
        return _matrix_bar("h", got_ret[0], want_ret[0], want_ret[2]) or _matrix_bar("s", got_ret[1], want_ret[1], want_ret[3])
    if n == "ritz" and got_ret["status"] == WAFER_OK:
        return _matrix_bar("h", got_ret["h"], want_ret["h"], want_ret["ah"]) or _matrix_bar("s", got_ret["s"], want_ret["s"], want_ret["as"])
    if solve:
        rows, wrows = got_ret[0], want_ret[0]
        if abs(len(rows) - len(wrows)) > 1:
            return "solve: %d rows against the oracle's %d" % (len(rows), len(wrows))
        for k, (g, w) in enumerate(zip(rows, wrows)):
            if g["step"] != w["step"] or g["tau"] != w["tau"]:
                return "solve row %d: step %r, tau %r against %r, %r" % (k, g["step"], g["tau"], w["step"], w["tau"])
            if not _close(g["energy"] / g["norm2"], w["energy"] / w["norm2"], abs_=SOLVE_E_ABS):
                return "solve row %d: E %r against %r" % (k, g["energy"] / g["norm2"], w["energy"] / w["norm2"])
            if not _close(np.sqrt(g["r2"] / g["norm2"]), np.sqrt(w["r2"] / w["norm2"]), rel=SOLVE_R_REL):
                return "solve row %d: r %r against %r" % (k, np.sqrt(g["r2"] / g["norm2"]), np.sqrt(w["r2"] / w["norm2"]))
    return None


def check_case(wa, wo, case, prog=None, mems=None):
    """one program on the device, every tier after every op; raises SequenceFailure at the first difference.  -> (ops, ops refused)"""
    from tests.test_gpu_batch import REL_SUM   # sums (observables, norm2) against the oracle
    seed, kind, ext, dtype = case
    prog = program(seed, kind, ext, dtype) if prog is None else prog
    mems = members(seed, kind, ext) if mems is None else mems
    B = len(mems)
    solos = [Solo(wa, mems, m, ext, dtype) for m in range(B)]
    ctxs = [FreeContext(wa, mems, m, ext, dtype) for m in range(B)] if not any(
        (op.name in ("evolve", "solve_state") and op.get("wnum")) or op.name == "orthogonalise" for op in prog if op.refused is None) else None
    models = [HostModel(wo, mem, ext) for mem in mems] if dtype == "f64" else None
    dev_norm2 = [None] * B

    def on_op(idx, op, before, after, ret):
        src = resolve_source(op, before, ext)
        for m in range(B):
            for tier, ex in (("T1 (the member alone in a Batch)", solos[m]), ("T2 (a free-running Context)", ctxs[m] if ctxs else None)):
                r = ex.step(op, src) if ex is not None else None
                if r is not None:
                    d = compare_exact(after[m], r[0])
                    if ex is not solos[m] and op.name == "norm2" and dtype == "f64":
                        # a Context's norm2 partitions an fp64 sum its own way: tests/test_gpu_batch_mixed.py holds the two to REL_SUM
                        # there and to equal bits on float storage.  Its next normalise divides by the batch's number, as the batch does.
                        d = d or (None if _close(ret[m], r[1], rel=REL_SUM) else "norm2: %r against %r" % (ret[m], r[1]))
                        ex.norm2 = ret[m]
                    else:
                        d = d or compare_exact(ret[m], r[1])
                    if d:
                        raise SequenceFailure(describe(case, prog, idx, m, tier, d))
            op1 = project(op, m, B, src)
            if models and op1 is not None:
                mod = models[m]
                mod.load(before[m])
                mod.norm2 = dev_norm2[m]
                want = mod.apply(op1, device=ret[m] if op.name == "ritz" else None)
                d = compare_oracle(op1, after[m], mod.snapshot(), ret[m], want, REL_SUM)
                if d:
                    raise SequenceFailure(describe(case, prog, idx, m, "T3 (the oracle, from the device's state before the op)", d))
        if op.name == "norm2":
            dev_norm2[:] = ret

    try:
        try:
            run_batch(wa, prog, mems, kind, ext, dtype, on_op)
        except SequenceFailure as e:
            if "replay:" in str(e):
                raise
            raise SequenceFailure("seed %d, kind %s, ext %d, dtype %s: %s\n%s" % (seed, kind, ext, dtype, e, "\n".join(
                "  %3d  %r" % (k, op) for k, op in enumerate(prog)))) from None
    finally:
        for ex in solos + (ctxs or []):
            ex.close()
    return len(prog), sum(op.refused is not None for op in prog)


def main(argv=None):
    ap = argparse.ArgumentParser(description="print one generated program of Batch calls (CPU only)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--kind", choices=KINDS, required=True)
    ap.add_argument("--ext", type=int, default=None, help="1, 2 or 3 (default: the one the committed case of this seed uses)")
    ap.add_argument("--dtype", choices=DTYPES, default="f64")
    ap.add_argument("--n-ops", type=int, default=N_OPS)
    args = ap.parse_args(argv)
    ext = seed_ext(args.seed) if args.ext is None else args.ext
    for k, mem in enumerate(members(args.seed, args.kind, ext)):
        print("member %d: %r" % (k, mem))
    for k, op in enumerate(program(args.seed, args.kind, ext, args.dtype, args.n_ops)):
        print("%3d  %r" % (k, op))


if __name__ == "__main__":
    main()

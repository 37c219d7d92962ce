//! Raw FFI to `libwafer_hip.so` (`include/wafer_hip.h`, ABI version 1) plus a thin safe wrapper
//! with the call shapes of Wafer's `grid.rs`.
//!
//! UNTESTED: no Rust toolchain exists in the image this engine was built in.  Struct layouts and
//! signatures mirror the C header field for field; `tests/test_abi.py` checks the same layout from
//! the Python side.
#![allow(non_camel_case_types)]
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_params {
    pub struct_size: u32,
    pub nx: u32,
    pub ny: u32,
    pub nz: u32,
    pub central_difference: i32, // CentralDifference::ext(): 1 | 2 | 3
    pub dtype: i32,              // 0 = f64, 1 = f32 storage
    pub dn: f64,
    pub dt: f64,
    pub mass: f64,
    pub sig: f64,
    pub max_states: u32,
    pub device: i32,
    pub z_begin: u32,
    pub z_count: u32,
    pub halo_depth: u32,
    pub flags: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_observables_t {
    pub energy: f64,
    pub norm2: f64,
    pub v_infinity: f64,
    pub r2: f64,
}

/// One row of the convergence table (grid.rs:126-221, output.rs:497-521).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_block_record {
    pub step: u64,
    pub tau: f64,
    pub obs: wafer_observables_t,
    pub diff: f64,
}

/// output.rs:32-45, 540-547
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_observables_output {
    pub state: u32,
    pub energy: f64,
    pub binding_energy: f64,
    pub r: f64,
    pub l_r: f64,
}

/// wafer_div_plan_t: how the step kernels divide by the run's stencil denominator (wafer_div_plan, wafer_get_div_plan)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_div_plan_t {
    pub den: f64,
    pub zh: f64,
    pub zl: f64,
    pub checked: i32,
    pub n_candidates: i32,
    pub zl_shift: i32,
    pub reserved: i32,
}

/// wafer_div_plan_f32_t: the same plan in fp32 (WAFER_F32_FAST contexts)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_div_plan_f32_t {
    pub den: f32,
    pub zh: f32,
    pub zl: f32,
    pub checked: i32,
    pub zl_shift: i32,
}

/// wafer_params.flags
pub const WAFER_FLAG_SKIP_DT_CHECK: u32 = 1;
pub const WAFER_FLAG_UNPLANNED_DIV: u32 = 2;
/// `target` / `src_kind` of `wafer_batch_resample(_member)`
pub const WAFER_RESAMPLE_PHI: c_int = 0;
pub const WAFER_RESAMPLE_POTENTIAL: c_int = 1;
pub const WAFER_RESAMPLE_POTSUB: c_int = 2;
pub const WAFER_RESAMPLE_STATE: c_int = 3;
/// `basis` of `wafer_batch_resample(_member)`: the member's padded size, or its work size
pub const WAFER_MOMENT_S: usize = 0;
pub const WAFER_MOMENT_X: usize = 1;
pub const WAFER_MOMENT_Y: usize = 2;
pub const WAFER_MOMENT_Z: usize = 3;
pub const WAFER_MOMENT_R2: usize = 4;
pub const WAFER_MOMENT_COUNT: usize = 5;

pub const WAFER_BASIS_PADDED: c_int = 0;
pub const WAFER_BASIS_WORK: c_int = 1;

/// wafer_peer_info (peer stores, wafer_set_overlap mode 3): what a rank publishes to its z-neighbours
#[repr(C)]
#[derive(Clone, Copy)]
pub struct wafer_peer_info {
    pub struct_size: u32,
    pub z_begin: u32,
    pub z_count: u32,
    pub halo_depth: u32,
    pub pid: u64,
    pub phi_addr: [u64; 2],
    pub flags_addr: u64,
    pub phi_alloc_offset: [u64; 2],
    pub phi_ipc: [[u8; 64]; 2],
    pub flags_ipc: [u8; 64],
    pub process_nonce: u64,
    pub device: i32,
    pub reserved: u32,
    pub device_uuid: [u8; 16],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct wafer_slab_info {
    pub z_begin: u32,
    pub z_count: u32,
    pub halo_depth: u32,
    pub ext: u32,
    pub plane_elems: u64,
    pub elem_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct wafer_device_info {
    pub name: [c_char; 64],
    pub arch: [c_char; 64],
    pub compute_units: u32,
    pub memory_clock_khz: u32,
    pub memory_bus_bits: u32,
    pub l2_bytes: u32,
    pub total_bytes: u64,
}

pub enum wafer_ctx {}
pub enum wafer_batch {}

pub type wafer_halo_fn = extern "C" fn(*mut c_void, *mut c_void, *mut c_void, *mut c_void, *mut c_void, usize, *mut c_void) -> c_int;
pub type wafer_allreduce_fn = extern "C" fn(*mut c_void, *mut c_void, usize, *mut c_void) -> c_int;

extern "C" {
    pub fn wafer_abi_version() -> c_int;
    pub fn wafer_last_error() -> *const c_char;
    pub fn wafer_ctx_create(p: *const wafer_params, out: *mut *mut wafer_ctx) -> c_int;
    pub fn wafer_ctx_destroy(ctx: *mut wafer_ctx) -> c_int;
    pub fn wafer_synchronize(ctx: *mut wafer_ctx) -> c_int;
    pub fn wafer_set_potential_builtin(ctx: *mut wafer_ctx, potential: c_int) -> c_int;
    pub fn wafer_set_potential_host(ctx: *mut wafer_ctx, v: *const f64, potsub_kind: c_int, potsub_scalar: f64, potsub: *const f64) -> c_int;
    pub fn wafer_set_initial_condition(ctx: *mut wafer_ctx, ic: c_int, seed: u64) -> c_int;
    pub fn wafer_upload_phi(ctx: *mut wafer_ctx, phi: *const f64) -> c_int;
    pub fn wafer_download_phi(ctx: *mut wafer_ctx, phi: *mut f64) -> c_int;
    pub fn wafer_download_phi_owned(ctx: *mut wafer_ctx, out: *mut f64) -> c_int;
    pub fn wafer_upload_phi_resampled(ctx: *mut wafer_ctx, src: *const f64, sx: u32, sy: u32, sz: u32, basis: *const u32) -> c_int;
    pub fn wafer_evolve(ctx: *mut wafer_ctx, wnum: u32, n_steps: u64) -> c_int;
    pub fn wafer_observables(ctx: *mut wafer_ctx, out: *mut wafer_observables_t) -> c_int;
    pub fn wafer_norm2(ctx: *mut wafer_ctx, out: *mut f64) -> c_int;
    pub fn wafer_normalise(ctx: *mut wafer_ctx, norm2: f64) -> c_int;
    pub fn wafer_orthogonalise(ctx: *mut wafer_ctx, wnum: u32) -> c_int;
    pub fn wafer_set_potsub(ctx: *mut wafer_ctx, kind: c_int, scalar: f64, potsub: *const f64) -> c_int;
    pub fn wafer_set_potsub_resampled(ctx: *mut wafer_ctx, src: *const f64, sx: u32, sy: u32, sz: u32) -> c_int;
    pub fn wafer_symmetrise(ctx: *mut wafer_ctx, constraint: c_int) -> c_int;
    pub fn wafer_push_state(ctx: *mut wafer_ctx) -> c_int;
    pub fn wafer_load_state(ctx: *mut wafer_ctx, idx: u32, state: *const f64) -> c_int;
    pub fn wafer_clone_state_to_phi(ctx: *mut wafer_ctx, idx: u32) -> c_int;
    pub fn wafer_set_comm_hooks(ctx: *mut wafer_ctx, halo: wafer_halo_fn, allreduce: wafer_allreduce_fn, user: *mut c_void) -> c_int;
    /// mode 0: exchange after the pass; 1: boundary planes first on a second stream; 2 (default): one launch per
    /// three-step pass, the slab as two halves marched outwards (include/wafer_hip.h)
    pub fn wafer_set_overlap(ctx: *mut wafer_ctx, mode: c_int) -> c_int;
    pub fn wafer_set_stream(ctx: *mut wafer_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn wafer_get_slab_info(ctx: *mut wafer_ctx, out: *mut wafer_slab_info) -> c_int;
    pub fn wafer_get_device_info(ctx: *mut wafer_ctx, out: *mut wafer_device_info) -> c_int;
    pub fn wafer_set_potential_resampled(ctx: *mut wafer_ctx, src: *const f64, sx: u32, sy: u32, sz: u32, basis: *const u32) -> c_int;
    pub fn wafer_download_array(ctx: *mut wafer_ctx, array_id: c_int, out: *mut f64) -> c_int;
    pub fn wafer_get_potsub(ctx: *mut wafer_ctx, kind: *mut c_int, scalar: *mut f64) -> c_int;
    pub fn wafer_download_state(ctx: *mut wafer_ctx, idx: u32, state: *mut f64) -> c_int;
    pub fn wafer_num_states(ctx: *mut wafer_ctx, out: *mut u32) -> c_int;
    pub fn wafer_clear_states(ctx: *mut wafer_ctx) -> c_int;
    /// Rayleigh-Ritz on the first k <= 8 (WAFER_RITZ_MAX) stored states (include/wafer_hip.h): row-major k * k matrices,
    /// coef[j * k + a] = component of input state j in output state a
    pub fn wafer_ritz_solve(k: u32, h: *const f64, s: *const f64, evals: *mut f64, coef: *mut f64) -> c_int;
    pub fn wafer_ritz_matrices(ctx: *mut wafer_ctx, k: u32, h: *mut f64, s: *mut f64) -> c_int;
    pub fn wafer_rotate_states(ctx: *mut wafer_ctx, k: u32, coef: *const f64) -> c_int;
    pub fn wafer_ritz(ctx: *mut wafer_ctx, k: u32, evals: *mut f64, coef: *mut f64, h: *mut f64, s: *mut f64) -> c_int;
    /// The first k stored states advanced by `n_steps` plain steps each (no projection, no normalisation): the bits of
    /// wafer_evolve(ctx, 0, n_steps) on each; phi and `cur` are left alone
    pub fn wafer_evolve_states(ctx: *mut wafer_ctx, k: u32, n_steps: u64) -> c_int;
    /// Host only: the coefficients of the scaled Chebyshev filter of `degree` steps that damps [a, b] and has magnitude 1 at a0 < a;
    /// `al`, `be` hold `degree` doubles, `cc` one
    pub fn wafer_filter_coefficients(degree: u32, a: f64, b: f64, a0: f64, al: *mut f64, be: *mut f64, cc: *mut f64) -> c_int;
    /// That polynomial of H applied to the first k stored states, one launch per state and step; phi and `cur` are left alone
    pub fn wafer_filter_states(ctx: *mut wafer_ctx, k: u32, degree: u32, a: f64, b: f64, a0: f64) -> c_int;
    /// Gershgorin's upper bound of H's spectrum: W / den + max V over the work cells
    pub fn wafer_spectral_bound(ctx: *mut wafer_ctx, ub: *mut f64) -> c_int;
    /// Residuals r = H l - theta l (include/wafer_hip.h): source 0 = the first k stored states, 1 = phi (k = 1); `theta_in` null is
    /// Rayleigh mode; `theta`, `r2`, `s` hold k doubles
    pub fn wafer_residuals(
        ctx: *mut wafer_ctx, source: c_int, k: u32, theta_in: *const f64, theta: *mut f64, r2: *mut f64, s: *mut f64,
    ) -> c_int;
    pub fn wafer_residual_to_phi(ctx: *mut wafer_ctx, idx: u32, theta: f64) -> c_int;
    /// The five moment matrices S, X, Y, Z, R2 of the first k stored states (include/wafer_hip.h; the origin lies one cell above the
    /// geometric centre, as in wafer_observables): `m` holds WAFER_MOMENT_COUNT * k * k doubles, m[(q * k + j) * k + i]
    pub fn wafer_moment_matrices(ctx: *mut wafer_ctx, k: u32, m: *mut f64) -> c_int;
    pub fn wafer_solve_state(
        ctx: *mut wafer_ctx, wnum: u32, tolerance: f64, screen_update: u64, has_max_steps: c_int, max_steps: u64,
        records: *mut wafer_block_record, max_records: usize, n_records: *mut usize, final_out: *mut wafer_observables_output,
    ) -> c_int;
    pub fn wafer_last_evolve_ms(ctx: *mut wafer_ctx, ms: *mut f32, steps: *mut u64) -> c_int;
    pub fn wafer_stencil_kernel_name(ctx: *mut wafer_ctx) -> *const c_char;
    pub fn wafer_stencil_kernel_instance(ctx: *mut wafer_ctx) -> *const c_char;
    pub fn wafer_stencil_steps_per_launch(ctx: *mut wafer_ctx) -> c_int;
    pub fn wafer_set_stencil_variant(ctx: *mut wafer_ctx, variant: c_int) -> c_int;
    pub fn wafer_set_halo_cycle(ctx: *mut wafer_ctx, passes: c_int) -> c_int;
    pub fn wafer_diag_copy_bw(ctx: *mut wafer_ctx, iters: c_int, unroll: c_int, blocks_per_cu: c_int, gbps: *mut f64) -> c_int;
    pub fn wafer_diag_checksum(ctx: *mut wafer_ctx, z_begin: u32, z_count: u32, out: *mut u64) -> c_int;
    /// which kernel a pass of `wafer_evolve(ctx, wnum, .)` launches, as one line of `key=value` pairs
    pub fn wafer_diag_dispatch(ctx: *mut wafer_ctx, wnum: u32, buf: *mut c_char, n: usize) -> c_int;
    /// padded planes [zp_begin, zp_begin + zp_count) of V / a / b (0 / 1 / 2) or phi (WAFER_ARRAY_PHI = 4), `[px][py][zp_count]`
    pub fn wafer_diag_download_window(ctx: *mut wafer_ctx, array_id: c_int, zp_begin: u32, zp_count: u32, out: *mut f64) -> c_int;
    pub fn wafer_diag_x2_passes(ctx: *mut wafer_ctx, out: *mut u64) -> c_int;
    pub fn wafer_peer_export(ctx: *mut wafer_ctx, out: *mut wafer_peer_info) -> c_int;
    pub fn wafer_peer_connect(ctx: *mut wafer_ctx, lower: *const wafer_peer_info, upper: *const wafer_peer_info) -> c_int;
    pub fn wafer_peer_disconnect(ctx: *mut wafer_ctx) -> c_int;
    pub fn wafer_diag_div_check(ctx: *mut wafer_ctx, den: f64, seed: u64, n_operands: u64, lo_exp: c_int, hi_exp: c_int, mismatches: *mut u64) -> c_int;
    pub fn wafer_div_plan(den: f64, out: *mut wafer_div_plan_t, candidates: *mut f64, cap: usize, n_written: *mut usize) -> c_int;
    pub fn wafer_get_div_plan(ctx: *mut wafer_ctx, out: *mut wafer_div_plan_t) -> c_int;
    pub fn wafer_div_plan_f32(den: f32, out: *mut wafer_div_plan_f32_t) -> c_int;
    pub fn wafer_diag_div_planned_f32(ctx: *mut wafer_ctx, plan: *const wafer_div_plan_f32_t, lo_exp: c_int, hi_exp: c_int, mismatches: *mut u64) -> c_int;
    pub fn wafer_diag_div_planned(ctx: *mut wafer_ctx, plan: *const wafer_div_plan_t, seed: u64, n_random: u64, lo_exp: c_int, hi_exp: c_int,
                                  operands: *const f64, n_operands: usize, mismatches_random: *mut u64, mismatches_operands: *mut u64) -> c_int;
    // batched ensembles: B ground-state problems of one shape and one dtype (WAFER_F64, WAFER_F32 or WAFER_F32_FAST in every member's
    // wafer_params), one launch per step (include/wafer_hip.h)
    pub fn wafer_batch_create(members: *const wafer_params, n_members: u32, out: *mut *mut wafer_batch) -> c_int;
    /// as `wafer_batch_create`, but nx, ny, nz may differ from member to member (ground-state calls; see wafer_hip.h)
    pub fn wafer_batch_create_mixed(members: *const wafer_params, n_members: u32, out: *mut *mut wafer_batch) -> c_int;
    pub fn wafer_batch_create_mixed_states(members: *const wafer_params, n_members: u32, out: *mut *mut wafer_batch) -> c_int;
    /// number of distinct (nx, ny, nz) among the members
    pub fn wafer_batch_num_shapes(b: *mut wafer_batch, n_shapes: *mut u32) -> c_int;
    pub fn wafer_batch_destroy(b: *mut wafer_batch) -> c_int;
    pub fn wafer_batch_size(b: *mut wafer_batch, n_members: *mut u32) -> c_int;
    pub fn wafer_batch_set_potential_builtin(b: *mut wafer_batch, member: u32, potential: c_int) -> c_int;
    pub fn wafer_batch_set_potential_host(b: *mut wafer_batch, member: u32, v: *const f64, potsub_kind: c_int, potsub_scalar: f64,
                                          potsub: *const f64) -> c_int;
    pub fn wafer_batch_set_initial_condition(b: *mut wafer_batch, member: u32, ic: c_int, seed: u64) -> c_int;
    pub fn wafer_batch_upload_phi(b: *mut wafer_batch, member: u32, phi: *const f64) -> c_int;
    pub fn wafer_batch_download_phi(b: *mut wafer_batch, member: u32, phi: *mut f64) -> c_int;
    pub fn wafer_batch_evolve(b: *mut wafer_batch, active: *const u8, n_steps: u64) -> c_int;
    pub fn wafer_batch_observables(b: *mut wafer_batch, out: *mut wafer_observables_t) -> c_int;
    pub fn wafer_batch_normalise(b: *mut wafer_batch, active: *const u8, norm2: *const f64) -> c_int;
    pub fn wafer_batch_solve(
        b: *mut wafer_batch, tolerance: f64, screen_update: u64, has_max_steps: c_int, max_steps: u64, records: *mut wafer_block_record,
        max_records_per_member: usize, n_records: *mut usize, finals: *mut wafer_observables_output, status: *mut c_int,
    ) -> c_int;
    pub fn wafer_batch_last_evolve_ms(b: *mut wafer_batch, ms: *mut f32, steps: *mut u64) -> c_int;
    pub fn wafer_batch_kernel_name(b: *mut wafer_batch) -> *const c_char;
    pub fn wafer_batch_steps_per_launch(b: *mut wafer_batch) -> c_int;
    pub fn wafer_batch_set_step_variant(b: *mut wafer_batch, variant: c_int) -> c_int;
    pub fn wafer_batch_diag_dispatch(b: *mut wafer_batch, buf: *mut c_char, n: usize) -> c_int;
    pub fn wafer_batch_diag_passes(b: *mut wafer_batch, fused_passes: *mut u64, single_steps: *mut u64) -> c_int;
    // batched excited states: per-member state stores and the normalise / Gram-Schmidt tail of every step
    pub fn wafer_batch_load_state(b: *mut wafer_batch, member: u32, idx: u32, state: *const f64) -> c_int;
    pub fn wafer_batch_download_state(b: *mut wafer_batch, member: u32, idx: u32, out: *mut f64) -> c_int;
    pub fn wafer_batch_push_state(b: *mut wafer_batch, active: *const u8) -> c_int;
    pub fn wafer_batch_num_states(b: *mut wafer_batch, counts_out: *mut u32) -> c_int;
    pub fn wafer_batch_clear_states(b: *mut wafer_batch, active: *const u8) -> c_int;
    pub fn wafer_batch_clone_state_to_phi(b: *mut wafer_batch, active: *const u8, idx: u32) -> c_int;
    pub fn wafer_batch_orthogonalise(b: *mut wafer_batch, active: *const u8, wnum: u32) -> c_int;
    pub fn wafer_batch_norm2(b: *mut wafer_batch, out: *mut f64) -> c_int;
    pub fn wafer_batch_evolve_state(b: *mut wafer_batch, active: *const u8, wnum: u32, n_steps: u64) -> c_int;
    pub fn wafer_batch_solve_state(
        b: *mut wafer_batch, wnum: u32, tolerance: f64, screen_update: u64, has_max_steps: c_int, max_steps: u64,
        records: *mut wafer_block_record, max_records_per_member: usize, n_records: *mut usize, finals: *mut wafer_observables_output,
        status: *mut c_int,
    ) -> c_int;
    pub fn wafer_batch_set_gs_variant(b: *mut wafer_batch, variant: c_int) -> c_int;
    pub fn wafer_batch_diag_gs(b: *mut wafer_batch, wnum: u32, buf: *mut c_char, n: usize) -> c_int;
    pub fn wafer_batch_diag_gs_steps(b: *mut wafer_batch, onepass: *mut u64, sequential: *mut u64) -> c_int;
    /// `wafer_symmetrise` for every active member in one launch, member m with `constraints[m]` (n_members entries, WAFER_SYM_*)
    pub fn wafer_batch_symmetrise(b: *mut wafer_batch, active: *const u8, constraints: *const c_int) -> c_int;
    /// `wafer_set_potsub` for one member
    pub fn wafer_batch_set_potsub(b: *mut wafer_batch, member: u32, kind: c_int, scalar: f64, potsub: *const f64) -> c_int;
    /// one host source (an unpadded `[sx][sy][sz]` array) resampled onto `target` (WAFER_RESAMPLE_*) of every active member in one launch
    pub fn wafer_batch_resample(b: *mut wafer_batch, active: *const u8, target: c_int, idx: u32, src: *const f64, sx: u32, sy: u32, sz: u32, basis: c_int) -> c_int;
    /// the same from the work cells of `src_member`'s phi (`src_kind` PHI) or stored state `src_idx` (STATE)
    pub fn wafer_batch_resample_member(b: *mut wafer_batch, active: *const u8, target: c_int, idx: u32, src_member: u32, src_kind: c_int, src_idx: u32, basis: c_int) -> c_int;
    /// HIP-event time of the last resample call's upload, transpose and launch
    pub fn wafer_batch_last_resample_ms(b: *mut wafer_batch, ms: *mut f32) -> c_int;
    /// set-up of every listed member (`active[m] != 0`, null: all) in one launch each; `potentials` / `ics` / `seeds`: `n_members` entries
    pub fn wafer_batch_set_potentials_builtin(b: *mut wafer_batch, active: *const u8, potentials: *const c_int) -> c_int;
    pub fn wafer_batch_set_initial_conditions(b: *mut wafer_batch, active: *const u8, ics: *const c_int, seeds: *const u64) -> c_int;
    /// `wafer_download_array` / `wafer_get_potsub` of one member
    pub fn wafer_batch_download_array(b: *mut wafer_batch, member: u32, array_id: c_int, out: *mut f64) -> c_int;
    pub fn wafer_batch_get_potsub(b: *mut wafer_batch, member: u32, kind: *mut c_int, scalar: *mut f64) -> c_int;
    pub fn wafer_batch_diag_member(b: *mut wafer_batch, member: u32, buf: *mut c_char, n: usize) -> c_int;
    pub fn wafer_batch_diag_setup_counts(b: *mut wafer_batch, launches: *mut u64, readbacks: *mut u64) -> c_int;
    /// Rayleigh-Ritz on the first `k[m]` stored states of every listed member (include/wafer_hip.h): `k` has n_members entries;
    /// `h`, `s`, `coef` hold member m's row-major k[m] x k[m] matrix at `m * 64` (WAFER_RITZ_MAX^2), `evals` its k[m] values at
    /// `m * 8`; `status` has n_members entries.  One sums launch, one reduce and one read-back for all members, one rotation launch.
    pub fn wafer_batch_ritz_matrices(b: *mut wafer_batch, active: *const u8, k: *const u32, h: *mut f64, s: *mut f64) -> c_int;
    pub fn wafer_batch_rotate_states(b: *mut wafer_batch, active: *const u8, k: *const u32, coef: *const f64) -> c_int;
    pub fn wafer_batch_ritz(
        b: *mut wafer_batch, active: *const u8, k: *const u32, evals: *mut f64, coef: *mut f64, h: *mut f64, s: *mut f64,
        status: *mut c_int,
    ) -> c_int;
    pub fn wafer_batch_diag_ritz_counts(b: *mut wafer_batch, launches: *mut u64, readbacks: *mut u64) -> c_int;
    /// wafer_residuals for every listed member: `theta_in`, `theta`, `r2`, `s` hold member m's k[m] values at `m * 8`
    pub fn wafer_batch_residuals(
        b: *mut wafer_batch, source: c_int, active: *const u8, k: *const u32, theta_in: *const f64, theta: *mut f64, r2: *mut f64,
        s: *mut f64, status: *mut c_int,
    ) -> c_int;
    pub fn wafer_batch_diag_residual_counts(b: *mut wafer_batch, launches: *mut u64, readbacks: *mut u64) -> c_int;
    /// wafer_moment_matrices for every listed member: member mb's matrix q, k[mb] x k[mb] row-major, at `(mb * 5 + q) * 64`
    pub fn wafer_batch_moment_matrices(b: *mut wafer_batch, active: *const u8, k: *const u32, m: *mut f64) -> c_int;
    pub fn wafer_batch_diag_moment_counts(b: *mut wafer_batch, launches: *mut u64, readbacks: *mut u64) -> c_int;
    /// wafer_evolve_states for every listed member with its own k[m] (0: nothing), one launch per step for all of them
    pub fn wafer_batch_evolve_states(b: *mut wafer_batch, active: *const u8, k: *const u32, n_steps: u64) -> c_int;
    pub fn wafer_batch_diag_store_step(b: *mut wafer_batch, buf: *mut c_char, n: usize) -> c_int;
    pub fn wafer_batch_diag_store_counts(b: *mut wafer_batch, launches: *mut u64) -> c_int;
    /// wafer_filter_states for every listed member with its own k[m] and interval, one launch per recurrence step for all of them
    pub fn wafer_batch_filter_states(
        b: *mut wafer_batch, active: *const u8, k: *const u32, degree: u32, a: *const f64, bb: *const f64, a0: *const f64,
    ) -> c_int;
    pub fn wafer_batch_spectral_bound(b: *mut wafer_batch, active: *const u8, ub: *mut f64) -> c_int;
    pub fn wafer_batch_diag_filter_counts(b: *mut wafer_batch, launches: *mut u64, bound_launches: *mut u64) -> c_int;
}

/// `Err(message)` for any non-zero status; a Wafer integration maps it to an `ErrorKind`.
pub fn check(rc: c_int) -> Result<(), String> {
    if rc == 0 {
        return Ok(());
    }
    let msg = unsafe { CStr::from_ptr(wafer_last_error()) }.to_string_lossy().into_owned();
    Err(format!("wafer_hip error {}: {}", rc, msg))
}

/// Device-resident solver state; method names follow `grid.rs`.
pub struct Engine {
    ctx: *mut wafer_ctx,
}

impl Engine {
    pub fn new(mut p: wafer_params) -> Result<Engine, String> {
        p.struct_size = std::mem::size_of::<wafer_params>() as u32;
        let mut ctx: *mut wafer_ctx = std::ptr::null_mut();
        check(unsafe { wafer_ctx_create(&p, &mut ctx) })?;
        Ok(Engine { ctx })
    }
    /// grid.rs:544-687
    pub fn evolve(&mut self, wnum: u8, steps: u64) -> Result<(), String> {
        check(unsafe { wafer_evolve(self.ctx, wnum as u32, steps) })
    }
    /// grid.rs:303-445
    pub fn compute_observables(&mut self) -> Result<wafer_observables_t, String> {
        let mut o = wafer_observables_t::default();
        check(unsafe { wafer_observables(self.ctx, &mut o) })?;
        Ok(o)
    }
    /// grid.rs:465-468
    pub fn normalise_wavefunction(&mut self, norm2: f64) -> Result<(), String> {
        check(unsafe { wafer_normalise(self.ctx, norm2) })
    }
    /// grid.rs:477-492
    pub fn orthogonalise_wavefunction(&mut self, wnum: u8) -> Result<(), String> {
        check(unsafe { wafer_orthogonalise(self.ctx, wnum as u32) })
    }
    /// `phi` is ndarray's standard-layout `Array3<R64>` storage, `(nx+bb, ny+bb, nz+bb)`.
    pub fn upload_phi(&mut self, phi: &[f64]) -> Result<(), String> {
        check(unsafe { wafer_upload_phi(self.ctx, phi.as_ptr()) })
    }
    pub fn download_phi(&mut self, phi: &mut [f64]) -> Result<(), String> {
        check(unsafe { wafer_download_phi(self.ctx, phi.as_mut_ptr()) })
    }
    /// One state of grid::solve (grid.rs:50-246): the evolve / observables / convergence loop on the
    /// device; `Ok(rows, summary)` when converged, the engine's MaxStep error otherwise.
    pub fn solve_state(
        &mut self, wnum: u8, tolerance: f64, screen_update: u64, max_steps: Option<u64>,
    ) -> Result<(Vec<wafer_block_record>, wafer_observables_output), String> {
        let mut rows = vec![wafer_block_record::default(); 4096];
        let mut n: usize = 0;
        let mut out = wafer_observables_output::default();
        check(unsafe {
            wafer_solve_state(
                self.ctx, wnum as u32, tolerance, screen_update, max_steps.is_some() as c_int, max_steps.unwrap_or(0),
                rows.as_mut_ptr(), rows.len(), &mut n, &mut out,
            )
        })?;
        rows.truncate(n);
        Ok((rows, out))
    }
    /// grid.rs:241
    pub fn push_state(&mut self) -> Result<(), String> {
        check(unsafe { wafer_push_state(self.ctx) })
    }
}

impl Drop for Engine {
    fn drop(&mut self) {
        unsafe { wafer_ctx_destroy(self.ctx) };
    }
}

/// `libwafer_rccl.so` (include/wafer_rccl.h): the halo / all-reduce hooks of a multi-GPU run served by RCCL's C API, for a
/// host that does not want to write them again, and the device-side all-reduce of the 1 + k sums
/// (include/wafer_mailbox.h, part of `libwafer_hip.so`).
#[repr(C)]
pub struct wafer_mailbox {
    _private: [u8; 0],
}

#[link(name = "wafer_rccl")]
extern "C" {
    pub fn wafer_rccl_last_error() -> *const c_char;
    pub fn wafer_rccl_unique_id_bytes() -> c_int;
    pub fn wafer_rccl_unique_id(out: *mut c_void) -> c_int;
    pub fn wafer_rccl_attach(
        ctx: *mut wafer_ctx, rank: c_int, world: c_int, unique_id: *const c_void, lower_override: c_int, upper_override: c_int,
        handle_out: *mut *mut c_void,
    ) -> c_int;
    pub fn wafer_rccl_warm_up(handle: *mut c_void, scratch: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn wafer_rccl_use_mailbox(handle: *mut c_void, mailbox: *mut c_void) -> c_int;
    pub fn wafer_rccl_allreduce_now(handle: *mut c_void, dev_ptr: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn wafer_rccl_halo_calls(handle: *mut c_void) -> std::os::raw::c_long;
    pub fn wafer_rccl_comm_info(
        handle: *mut c_void, nranks: *mut c_int, rank: *mut c_int, lower: *mut c_int, upper: *mut c_int, version: *mut c_int,
    ) -> c_int;
    pub fn wafer_rccl_detach(ctx: *mut wafer_ctx, handle: *mut c_void) -> c_int;
}

#[link(name = "wafer_hip")]
extern "C" {
    pub fn wafer_mailbox_create(rank: c_int, world: c_int, device: c_int, out: *mut *mut wafer_mailbox) -> c_int;
    pub fn wafer_mailbox_handle(mb: *mut wafer_mailbox, handle_out: *mut c_void) -> c_int;
    pub fn wafer_mailbox_connect(mb: *mut wafer_mailbox, all_handles: *const c_void) -> c_int;
    pub fn wafer_mailbox_allreduce(mailbox: *mut c_void, dev_ptr: *mut c_void, count: usize, hip_stream: *mut c_void) -> c_int;
    pub fn wafer_mailbox_check(mb: *mut wafer_mailbox) -> c_int;
    pub fn wafer_mailbox_destroy(mb: *mut wafer_mailbox) -> c_int;
}

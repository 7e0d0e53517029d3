"""CPU: which launch sequence of the first-task program (T0Plan, csrc/elbo_t0.hip) the shapes of the GPU tests take.

The GPU tests reach the program's paths by choosing shapes and naming the intended path in a comment; the plan depends on the CU
count and on thresholds that performance work retunes, so a shape can move to another path while its comparison with the oracle
still passes.  `vargp_elbo_t0_plan` (fused.t0_plan) evaluates the library's own t0_plan on the host; here, for the 256 CUs of an
MI355X:
  a. the comment of every shape group of test_hip_t0_program / test_hip_front_roles / test_hip_fold_small /
     test_hip_trainer_edges as an assertion on the plan's flags;
  b. a coverage condition over the shapes that are compared with the oracle: on the route of VARGP.loss and on the trainer's
     (defer_softmax requested) every flag of the plan is true for one shape and false for another, and the deferred likelihood
     meets every launch sequence around it;
  c. the host rules Python mirrors or relies on: VARGP.first_task_as_block against fused_mid / fused_bwd, and the range of
     fwd_parts / bwd_parts."""
import pytest
import torch

import test_hip_fold_small as fold
import test_hip_front_roles as front
import test_hip_t0_program as t0p
import test_hip_trainer_edges as edges
from vargp_amd import fused

CUS = 256


def plan(shape, cus=CUS, **flags):
    S, F_, C, M, D, B = shape
    return fused.t0_plan(S, C, M, D, B, F_, cus=cus, **flags)


def test_query_returns_every_member_and_needs_no_device():
    p = plan((3, 10, 10, 100, 784, 512), defer_softmax=True)
    bools = ['native', 'generic_lik', 'unscaled_lik_grad', 'defer_softmax', 'fwd_softmax16', 'direct_gram', 'merge_chol', 'split_kuu',
             'front', 'gram_in_chain', 'su_in_chain', 'fused_mid', 'fwd_multi', 'w_vec4', 'unmerge', 'side', 'fused_bwd', 'mat_bwd',
             'bwd_multi', 'fused_tail', 'tail_lds', 'fold_small']
    ints = ['kuf_tile', 'puf_tile', 'puu_tile', 'fold_roles', 'fold_extra', 'ksp', 'ntile', 'fwd_parts', 'bwd_parts']
    assert sorted(p) == sorted(bools + ints)
    assert all(type(p[k]) is bool for k in bools) and all(type(p[k]) is int for k in ints)
    # the benchmark's step (BASELINE config 2): eight launches -- front launch, merged factorisation, folded single-tile middles,
    # the likelihood inside the backward's tile kernel, per-matrix chains beside P_uf, the fused tail
    on = {k for k in bools if p[k]}
    assert on == {'unscaled_lik_grad', 'defer_softmax', 'merge_chol', 'split_kuu', 'front', 'su_in_chain', 'fused_mid', 'w_vec4',
                  'fused_bwd', 'mat_bwd', 'fused_tail', 'fold_small'}, on
    assert (p['ntile'], p['fwd_parts'], p['bwd_parts'], p['ksp']) == (8, 8, 8, 2)
    # flags of the descriptor
    assert plan((2, 2, 2, 20, 36, 64), native=True)['native'] and not plan((2, 2, 2, 20, 36, 64))['native']
    ext = plan((2, 2, 2, 20, 36, 64), ext_lik=True, defer_softmax=True)
    assert not (ext['native'] or ext['unscaled_lik_grad'] or ext['generic_lik'] or ext['defer_softmax'] or ext['fwd_softmax16'])


def test_query_rejects_bad_arguments():
    import ctypes
    from vargp_amd._lib import ElboT0Desc, VargpHipError, lib
    with pytest.raises(VargpHipError, match='bad dims'):
        fused.t0_plan(1, 1, 0, 4, 4, 1, cus=CUS)
    desc = ElboT0Desc(S=1, C=1, M=4, D=4, B=4, F=1)
    small = ctypes.create_string_buffer(16)
    assert lib().vargp_elbo_t0_plan(ctypes.byref(desc), CUS, small, len(small)) != 0
    assert b'bytes' in lib().vargp_last_error()
    assert lib().vargp_elbo_t0_plan(None, CUS, small, len(small)) != 0


# ---- a. the comments of the shape lists as assertions ------------------------------------------------------------------------
# flags: 'name' must be true, '!name' false (test_hip_trainer_edges.flags_of)
T0_PROGRAM_GROUPS = [
    ('odd M: padded small-column block, no LDS-resident kernels', [(2, 3, 3, 33, 40, 50)], '!fused_mid !fused_bwd !w_vec4'),
    ('B % 4 != 0: no float4 rows of W', [(3, 2, 4, 20, 64, 37)], 'fused_mid !w_vec4 !fused_bwd'),
    ('C > 16: the generic softmax kernels', [(2, 2, 18, 12, 36, 24)], 'generic_lik !unscaled_lik_grad !fwd_softmax16'),
    ('D <= 32: the direct distance form', [(2, 3, 2, 20, 2, 64)], 'direct_gram !merge_chol'),
    ('M > 100: the blocked Cholesky', [(1, 2, 2, 130, 48, 40)], '!merge_chol !fused_mid !fused_bwd'),
    ('tiny / degenerate', [(1, 1, 1, 3, 33, 2)], '!merge_chol !fused_mid !fused_bwd'),
    ('M = 64 / 65 / 100 / 51: the factorisation kernel of the merged launch',
     [(2, 2, 2, 64, 40, 33), (2, 2, 2, 65, 40, 32), (1, 2, 2, 100, 36, 50), (1, 2, 3, 51, 36, 8)], 'merge_chol !fused_bwd'),
    ('the LDS-resident backward with the per-matrix chains and the fused tail',
     [(3, 2, 3, 100, 40, 72), (4, 2, 2, 104, 36, 64), (5, 2, 2, 52, 36, 40), (2, 2, 2, 4, 36, 8), (2, 3, 3, 96, 48, 200),
      (3, 2, 2, 100, 36, 132), (8, 2, 2, 100, 36, 64), (16, 1, 2, 100, 36, 64), (17, 2, 2, 52, 36, 40)],
     'fused_mid fused_bwd mat_bwd fused_tail !fwd_multi !bwd_multi !unmerge'),
    ('... its tail with the per-sample operands staged through LDS (S > 4)',
     [(5, 2, 2, 52, 36, 40), (8, 2, 2, 100, 36, 64), (16, 1, 2, 100, 36, 64), (17, 2, 2, 52, 36, 40)], 'tail_lds'),
    ('the persistent P_uf role of the merged launch', [(3, 2, 10, 100, 784, 256), (3, 2, 10, 100, 784, 320), (7, 2, 10, 100, 448, 256)],
     'mat_bwd !unmerge front'),
    ('the multi-tile form of the tile kernels', [(8, 2, 10, 100, 36, 512), (6, 2, 10, 96, 36, 328), (12, 1, 9, 100, 36, 200),
                                                 (16, 1, 16, 100, 36, 128)], 'fwd_multi bwd_multi'),
    ('... with B % 4 != 0 (the forward alone)', [(10, 2, 10, 52, 36, 130)], 'fwd_multi !fused_bwd !w_vec4'),
    ('the role-merged launches taken apart', [(17, 1, 16, 52, 36, 64), (33, 1, 8, 100, 36, 72)], 'unmerge side merge_chol mat_bwd'),
    ('... behind the front launch, Gram matrices built by the chain workgroups', [(13, 1, 10, 100, 256, 128)],
     'unmerge side front gram_in_chain'),
    ('the tile kernels WITHOUT the per-matrix chains / fused tail', [(3, 2, 2, 52, 38, 40), (65, 1, 2, 52, 36, 40)],
     'fused_bwd !mat_bwd !fused_tail'),
]


def _assert_flags(shape, want, what, **flags):
    p = plan(shape, **flags)
    bad = {k: v for k, v in edges.flags_of(want).items() if p[k] != v}
    assert not bad, f'{shape} ({what}): at {CUS} CUs the plan does not show {bad}: {p}'
    return p


@pytest.mark.parametrize('what,shapes,want', T0_PROGRAM_GROUPS, ids=[g[0] for g in T0_PROGRAM_GROUPS])
def test_t0_program_shapes_take_the_paths_their_comments_name(what, shapes, want):
    for shape in shapes:
        assert shape in t0p.SHAPES, f'{shape} is no longer in test_hip_t0_program.SHAPES: move its assertion with it'
        _assert_flags(shape, want, what)


def test_t0_program_groups_cover_the_whole_list():
    grouped = {s for _, shapes, _ in T0_PROGRAM_GROUPS for s in shapes}
    assert grouped == set(t0p.SHAPES), set(t0p.SHAPES) ^ grouped
    # multi-tile forms: uneven tile shares (8 tiles over 3 workgroups), one workgroup for all tiles of a matrix
    p = plan((8, 2, 10, 100, 36, 512))
    assert (p['ntile'], p['fwd_parts'], p['bwd_parts']) == (8, 3, 3)
    p = plan((16, 1, 16, 100, 36, 128))
    assert (p['ntile'], p['fwd_parts'], p['bwd_parts']) == (2, 1, 1)


def test_front_roles_shapes_take_the_paths_their_comments_name():
    for shape in front.SHAPES:
        M, D = shape[3], shape[4]
        if D == 32:       # the tile kernels (every streamed output), neither the front launch nor the merged factorisation launch
            _assert_flags(shape, 'direct_gram fused_mid fused_bwd !front !merge_chol !su_in_chain', 'D = 32')
        else:             # the eight-launch step of the benchmark
            _assert_flags(shape, 'front merge_chol fused_mid fused_bwd mat_bwd fused_tail fold_small !unmerge', 'D = 256')
            _assert_flags(shape, 'su_in_chain' if shape in front.FRONT_SHAPES else '!su_in_chain', 'S_u by its chain: 64 < M <= 100')
    assert front.FRONT_SHAPES and all(s[3] > 64 for s in front.FRONT_SHAPES)
    # test_unmerged_plan_still_builds_su_in_its_chain, as it sizes S on a 256-CU device
    S = (CUS // 2) // 3 + 1
    _assert_flags((S, 1, 3, 68, 256, 64), 'unmerge side su_in_chain front', 'unmerged, S_u in its chain')


def test_fold_small_shapes_fold():
    two_matrix_roles = 0
    for case in fold.CASES:
        p = _assert_flags(case, 'fold_small fused_mid !fwd_multi direct_gram', 'folded small-column product')
        S, C = case[0], case[2]
        assert p['fold_roles'] >= (S * C + 1) // 2          # role workgroups take at most two matrices each
        two_matrix_roles += p['fold_roles'] < S * C
    assert two_matrix_roles                                # ... and somewhere they do take two


@pytest.mark.parametrize('shape,map_est,want', edges.EDGES, ids=edges.IDS)
def test_trainer_edge_shapes_take_the_paths_they_name(shape, map_est, want):
    _assert_flags(shape, want + ' !native', 'trainer route', defer_softmax=True, map_est=map_est)
    if shape in [e[0] for e in edges.NATIVE]:
        _assert_flags(shape, want + ' native defer_softmax', 'trainer route, native noise', defer_softmax=True, native=True)


# ---- b. coverage as a condition ----------------------------------------------------------------------------------------------
# What is compared with the oracle on each route: (shape, descriptor flags).  The route of VARGP.loss never requests defer_softmax
# (that is the trainer's); everything else can vary on both.
BENCH = (3, 10, 10, 100, 784, 512)                  # test_hip_timed_route: smnist_full_t0
LOSS_ROUTE = ([(s, {}) for s in t0p.SHAPES + t0p.RANDOM_SHAPES + front.SHAPES + fold.CASES]
              + [(edges.LOSS_NATIVE, dict(native=True))])
TRAINER_ROUTE = ([(s, dict(defer_softmax=True, map_est=m)) for s, m, _ in edges.EDGES]
                 + [(s, dict(defer_softmax=True, native=True)) for s, _, _ in edges.NATIVE]
                 + [(BENCH, dict(defer_softmax=True)), ((16, 2, 16, 32, 40, 64), dict(defer_softmax=True))])
TRAINER_PAIRS = [('defer_softmax', 'front'), ('defer_softmax', 'unmerge'), ('defer_softmax', '!mat_bwd'), ('defer_softmax', 'direct_gram'),
                 ('defer_softmax', 'native'), ('!defer_softmax', 'bwd_multi'), ('!defer_softmax', 'generic_lik')]


def _table(route):
    plans = [(shape, plan(shape, **flags)) for shape, flags in route]
    names = [k for k, v in plans[0][1].items() if type(v) is bool]
    return plans, names


def _print_table(title, plans, names):
    print(f'\n{title}: {len(plans)} cases at {CUS} CUs')
    for k in names:
        yes = [s for s, p in plans if p[k]]
        print(f'  {k:18s} true {len(yes):3d}  false {len(plans) - len(yes):3d}   e.g. true {yes[0] if yes else "-"}, false '
              f'{next((s for s, p in plans if not p[k]), "-")}')


def test_every_flag_is_compared_with_the_oracle_both_ways_on_both_routes():
    for title, route, fixed in (('route of VARGP.loss', LOSS_ROUTE, {'defer_softmax'}), ("the trainer's route", TRAINER_ROUTE, set())):
        plans, names = _table(route)
        _print_table(title, plans, names)
        one_sided = [k for k in names if k not in fixed and len({p[k] for _, p in plans}) != 2]
        assert not one_sided, f'{title}: no shape compared with the oracle has these flags both true and false: {one_sided}'
        assert all(not p[k] for k in fixed for _, p in plans)
    plans, _ = _table(TRAINER_ROUTE)
    has = lambda p, w: p[w.lstrip('!')] != w.startswith('!')
    for a, b in TRAINER_PAIRS:
        hit = [s for s, p in plans if has(p, a) and has(p, b)]
        print(f'  {a} with {b}: {hit}')
        assert hit, f"the trainer's route: no shape with {a} and {b}"
    hit = [s for s, p in plans if not p['defer_softmax'] and p['fused_bwd'] and p['unscaled_lik_grad'] and s[1] > 16]
    print(f'  !defer_softmax with fused_bwd because F > 16: {hit}')
    assert hit


# ---- c. host rules Python mirrors --------------------------------------------------------------------------------------------
def test_first_task_as_block_agrees_with_the_plan():
    """VARGP.first_task_as_block: "outside the range of the LDS-resident middles (M <= 104 and at most 16384 tile units)" -- so,
    where the middles' other conditions hold (M % 4 == 0, M >= 4, B % 4 == 0), exactly where the plan has neither of them; and
    nowhere else does it send a shape to the block program that the plan would give a middle."""
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    limit = VARGP.T0_TILE_UNITS_MAX
    assert limit == 16384
    grid = [(S, C, M, B) for M in (4, 100, 102, 104, 105, 108) for (S, C, B) in
            [(1, 1, 4), (3, 10, 512), (1024, 2, 512), (2047, 1, 512), (2048, 1, 512), (2049, 1, 512), (683, 3, 512), (2048, 1, 516),
             (2048, 1, 448), (2341, 1, 448), (2340, 1, 448), (16384, 1, 64), (16385, 1, 64), (16384, 1, 68), (8192, 2, 64),
             (8192, 2, 62), (5462, 3, 60), (5461, 3, 64), (103, 1, 104 * 64), (104, 1, 157 * 64), (104, 1, 158 * 64)]]
    seen = set()
    for S, C, M, B in grid:
        gp = VARGP(torch.zeros(C, M, 4), RBFKernel(4), MulticlassSoftmax(n_f=1), n_var_samples=S)
        block = gp.first_task_as_block(B)
        p = plan((S, 1, C, M, 4, B))
        middles = p['fused_mid'] or p['fused_bwd']
        assert not (block and middles), (S, C, M, B, p)
        if M % 4 == 0 and B % 4 == 0:
            assert block == (not middles), (S, C, M, B, block, p)
            seen.add((block, M > 104, S * C * ((B + 63) // 64) > limit))
    assert seen == {(False, False, False), (True, True, False), (True, False, True), (True, True, True)}, seen


@pytest.mark.parametrize('cus', [64, 256, 304])
def test_tile_parts_stay_in_range(cus):
    for SC in (1, 2, 7, 30, 63, 64, 65, 100, 255, 256, 257, 304, 305, 1000, 2048):
        for ntile in (1, 2, 3, 4, 5, 8, 9, 16, 33):
            S, C = (SC, 1) if SC % 2 else (SC // 2, 2)
            p = plan((S, 1, C, 20, 36, 64 * ntile - 4), cus=cus)
            assert p['ntile'] == ntile
            for k in ('fwd_parts', 'bwd_parts'):
                assert 1 <= p[k] <= ntile, (SC, ntile, cus, p)
                if SC * ntile <= cus:
                    assert p[k] == ntile, (SC, ntile, cus, p)
            assert p['fwd_multi'] == (p['fwd_parts'] < ntile) and p['bwd_multi'] == (p['fused_bwd'] and p['bwd_parts'] < ntile)

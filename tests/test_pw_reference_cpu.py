"""CPU: the float64 references of the point-wise head kernels and the backbone seams (tests/pw_cases.py), the conditions on
the cases that the GPU sweep (tests/test_pw_sweep_gpu.py) relies on, and the sensitivity of the comparison functions both
tests share.

For every stage a torch emulation of the kernel's partitioning passes the comparison function under the derived bound, and
every defect of pw_cases.MUTANTS fails it on a named case: the case list cannot quietly lose its edge.  What is proven
here about the checks holds on the GPU, which calls the same functions.
"""
import pytest
import torch

from tests import pw_cases as P


def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _gemm(name, mutant=None, job0=None):
    j = P.GEMM_BY_NAME[name]
    B, L = P.gemm_columns(j)
    ops = P.gemm_operands(name, B, L)
    full, stats = P.emulate_gemm(j, ops, B, L, mutant, job0)
    return j, ops, full, stats


def _gemm_rejects(name, mutant, job0=None):
    j, ops, full, stats = _gemm(name, mutant, job0)
    return _caught(lambda: P.check_gemm(j, ops, P.gemm_out_slice(j, full), stats))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def test_gemm_job_list_reaches_every_branch():
    jobs = P.GEMM_JOBS
    assert 30 <= len(jobs) <= 40 and len({j.name for j in jobs}) == len(jobs)
    br = {j.name: P.gemm_branches(j) for j in jobs}
    assert {j.K for j in jobs if not j.w_t} == set(P.K_ROW_MAJOR) and all(j.K % 16 == 0 for j in jobs if not j.w_t)
    assert {j.K for j in jobs if j.w_t} == set(P.K_TRANSPOSED)
    assert {j.rows for j in jobs} == set(P.GEMM_ROWS)
    assert {P.gemm_columns(j) for j in jobs} == set(P.COLUMNS)
    # the weight pipeline: one group exactly, the c0 + 4 and c0 + 8 branches taken and not taken, the LDS opt-in
    assert {4, 5, 9, 12, 13, 35} <= {b["nch"] for b in br.values()}
    assert br["f560x256"]["nch"] == br["t547x63"]["nch"] == 35 == P.PW_KMAX // 16
    assert br["f64x257"]["mtiles"] == 17 and br["f64x257"]["second_trip"] and not br["f560x256"]["second_trip"]
    assert br["f16x1"]["dead_waves"] == 3 and br["f64x15"]["dead_waves"] == 3 and br["f80x16"]["dead_waves"] == 3
    assert {b["dead_waves"] for b in br.values()} >= {0, 2, 3}
    # NLC input: the 16-byte path and both scalar triggers; NLC output: float4 and its three off-conditions
    assert {(b["x_path"], b["scalar_why"]) for b in br.values()} >= {("ncl", None), ("vec", None), ("scalar", "k"), ("scalar", "ctot")}
    assert br["f192x64"]["x_path"] == "vec" and br["t3x64"]["scalar_why"] == "k" and br["f64x16_xodd"]["scalar_why"] == "ctot"
    assert {(b["out_path"], b["out_why"]) for b in br.values()} >= {("ncl", None), ("vec", None), ("scalar", "rows"),
                                                                    ("scalar", "ctot"), ("scalar", "ptr")}
    assert br["f192x64"]["out_path"] == "vec" and br["f64x64_octot"]["out_why"] == "ctot" and br["f64x64_off4"]["out_why"] == "ptr"
    assert {j.tr for j in jobs} == {0, 1, 2} and {j.epi for j in jobs} == {0, 1}
    assert {(j.epi, j.stats) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {j.bias for j in jobs} == {0, 1}
    assert any(j.xs and j.xc0 and not j.x_nlc for j in jobs) and any(j.xs and j.xc0 and j.x_nlc for j in jobs)
    assert any(j.os and j.oc0 and not j.out_nlc for j in jobs) and any(j.os and j.oc0 and j.out_nlc for j in jobs)
    assert any(j.ms and j.mc0 for j in jobs) and any(j.ld and j.tr for j in jobs) and any(j.ld and j.epi for j in jobs)
    assert any(j.w_t and P.kpad_of(j.K) > j.K and j.K % 16 == 15 for j in jobs)          # the clamp of kk at K - 1
    for n, ((B, L), names) in P.GEMM_LISTS.items():
        assert len(names) == n and (B, L) in P.COLUMNS
        lj = [P.GEMM_BY_NAME[x] for x in names]
        assert len({j.K for j in lj}) >= n - 1 and len({j.rows for j in lj}) >= n - 2
        assert {j.w_t for j in lj} == {0, 1} or n == 2
        assert max(P.kpad_of(j.K) for j in lj) > P.kpad_of(lj[0].K)      # the LDS tile is sized by a later job of the list
    assert {"f16x1", "f560x256"} == set(P.GEMM_LISTS[2][1])


def test_wgrad_and_reduce_cases():
    jobs = P.WGRAD_JOBS
    assert {j.rows for j in jobs} == set(P.WGRAD_DIMS) == {j.K for j in jobs}
    assert {(j.x_nlc, j.y_nlc) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {j.tr for j in jobs} == {0, 2} and {j.ytr for j in jobs} == {0, 1} and {j.db for j in jobs} == {0, 1}
    vec = lambda n, ct: ((n | ct) & 3) == 0
    assert {vec(j.rows, j.rows + j.xs) for j in jobs if j.x_nlc} == {True, False}
    assert {vec(j.K, j.K + j.ys) for j in jobs if j.y_nlc} == {True, False}
    assert max(((j.rows + 63) // 64) * ((j.K + 63) // 64) for j in jobs) == 9
    assert [B * L // 64 for B, L in P.WGRAD_COLUMNS] == [1, 3, 4]
    assert P.wgrad_ranges(3, 2) == [(0, 2), (2, 3)]                  # at L = 64 the first range crosses a sample boundary
    assert P.wgrad_ranges(3, 4)[-1] == (3, 3) and P.wgrad_ranges(1, 2) == [(0, 1), (1, 1)]       # ranges with no chunk
    assert P.wgrad_ranges(4, 3) == [(0, 2), (2, 4), (4, 4)]
    for n, ((B, L), entries) in P.WGRAD_LISTS.items():
        tiles = [((P.WGRAD_BY_NAME[x].rows + 63) // 64) * ((P.WGRAD_BY_NAME[x].K + 63) // 64) * sp for x, sp in entries]
        assert len(entries) == n and len(set(tiles)) >= 3
    assert P.REDUCE_P == (1, 2, 3, 4, 5, 7, 8, 9) and P.REDUCE_M == (1, 255, 256, 257, 513)
    assert {p % 4 for p in P.REDUCE_P} == {0, 1, 2, 3}


def test_finalize_and_mix_cases():
    assert P.FIN_P == (1, 63, 64, 65, 130) and P.FIN_C == (1, 5, 96) and P.FIN_MOMENTUM == (0.1, 1.0, 0.0, -1.0)
    c = P.finalize_case(65, 5)
    assert c["part"][:, 0, 0].unique().numel() > 5                                 # unequal counts
    for Pn in P.FIN_P:
        ref = P.finalize_ref(P.finalize_case(Pn, 5, "big"), 0.1)["out"][0]
        ratio = ref[0].abs() * ref[1]
        assert (ratio > 100).all() and (ratio < 1e4).all()
        const = P.finalize_ref(P.finalize_case(Pn, 5, "const"), 0.1)["out"][0]
        assert const[1, 0] == (torch.tensor(P.EPS, dtype=torch.float64)).rsqrt() and const[0, 0] == 0.7109375
    assert [B * L for B, L in P.MIX_COLS] == [1, 15, 16, 17, 111, 257, 600] and P.MIX_G == (1, 15, 16, 17, 100)
    assert {h.D for h in P.MIX_LAUNCH} == {1, 2, 3, 4} and {h.f64 for h in P.MIX_LAUNCH} == {0, 1}
    assert {(h.D, h.f64) for launch in P.MIX_LAUNCHES for h in launch} == {(D, t) for D in P.MIX_D for t in (0, 1)}
    assert all({h.eps for h in launch} == {0, 1} for launch in P.MIX_LAUNCHES)
    assert P.EXPF_ULP >= 2 and P.EXPF_ULP >= 2 * P.PI_ULP_MEASURED


def test_seam_cases():
    assert [C * J for C, J in P.GATHER_CJ] == [1, 255, 256, 257]
    i40, i130 = P.designed_inds_40(), P.designed_inds_130()
    assert i40.shape == (1, 40) and i130.shape == (1, 130)
    h40 = P.hit_counts(i40, 13)[0].tolist()
    assert h40[:6] == [17, 16, 3, 2, 1, 0] and h40[12] == 1 and sum(h40) == 40      # > 16, == 16, > 2, == 2, 1, 0; ragged chunk
    h130 = P.hit_counts(i130, 13)[0].tolist()
    assert h130[3] == 5 and h130[9] == 17 and max(h for t, h in enumerate(h130) if t != 9) <= 5
    assert (i130[0] == 3).nonzero().flatten().tolist() == [0, 63, 64, 65, 129]
    assert P.ballot_trips(i130, 3) == [0, 1, 2] and P.ballot_trips(i130, 9) == [0, 1, 2]
    assert int(i130[0, 5]) == -1 and int(i130[0, 70]) == 13 and int(((i130 < 0) | (i130 >= 13)).sum()) > 50
    # the 17th seed of frame 9 comes from the third trip: the list is full before it
    assert sum(1 for s in (i130[0] == 9).nonzero().flatten().tolist() if s < 128) == 16
    assert P.PREFIX_T == (1, 2, 255, 257, 16384, 16385, 40000) and P.PREFIX_S == (1, 255, 256, 257)
    cum, target = P.prefix_case(2, 257, 257)
    d = (cum[:, :, None] - target[:, None, :]).abs()
    ties = (d == d.min(1, keepdim=True).values).sum(1)
    assert (ties > 1).any(), "no plateau or mid-point tie in the case"
    assert (torch.diff(cum, dim=1) == 0).any()


# ---- the emulators pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [j.name for j in P.GEMM_JOBS])
def test_emulated_gemm(name):
    j, ops, full, stats = _gemm(name)
    ratios = P.check_gemm(j, ops, P.gemm_out_slice(j, full), stats)
    assert (stats is not None) == bool(j.stats)
    written = ~torch.isnan(full)
    assert int(written.sum()) == j.rows * full.numel() // (j.rows + j.os)          # the slice and nothing else
    print(name, ratios)


@pytest.mark.parametrize("name", [j.name for j in P.WGRAD_JOBS])
def test_emulated_wgrad(name):
    j = P.WGRAD_BY_NAME[name]
    for B, L in P.WGRAD_COLUMNS:
        chunks = B * L // 64
        ops = P.wgrad_operands(name, B, L)
        for split in P.wgrad_splits(chunks):
            dw, db = P.emulate_wgrad(j, ops, chunks, split)
            P.check_wgrad(j, dw, db, P.wgrad_ref(j, ops, chunks, split), chunks, split)


def test_emulated_reduce():
    for Pn in P.REDUCE_P:
        for M in P.REDUCE_M:
            inp = P.reduce_case(Pn, M)
            P.check_bound(P.emulate_reduce(inp), P.reduce_ref(inp), f"P {Pn} M {M}")


@pytest.mark.parametrize("kind", P.FIN_KINDS)
@pytest.mark.parametrize("Pn", P.FIN_P)
def test_emulated_finalize(Pn, kind):
    for C in P.FIN_C:
        case = P.finalize_case(Pn, C, kind)
        for momentum in P.FIN_MOMENTUM:
            got = P.emulate_finalize(case, momentum)
            P.check_finalize(got, P.finalize_ref(case, momentum), f"P {Pn} C {C} {kind} momentum {momentum}")
            if kind == "const":
                assert got["out"][1, 0] == torch.tensor(1.0 / P.EPS ** 0.5, dtype=torch.float64).float()
        part, fin, M = P.bwd_finalize_case(Pn, C)
        for train in (1, 0):
            P.check_bwd_finalize(P.emulate_bwd_finalize(part, fin, M, train), P.bwd_finalize_ref(part, fin, M, train), f"P {Pn} C {C}")


@pytest.mark.parametrize("B,L", P.MIX_COLS)
def test_emulated_mix(B, L):
    for G in P.MIX_G:
        for D, f64 in sorted({(h.D, h.f64) for launch in P.MIX_LAUNCHES for h in launch}):
            c = P.mix_case(B, L, G, D, f64)
            for with_eps in (True, False):
                pred, pi = P.emulate_mix_forward(c, with_eps)
                P.check_bound_any(pred, P.mix_forward_ref(c, with_eps), f"{(B, L, G, D, f64)} pred")
                P.check_bound(pi, P.pi_ref(c), "pi")
                assert P.pi_ulps(pi, c) <= P.EXPF_ULP
            dl, dmu, dls = P.emulate_mix_backward(c)
            ref = P.mix_backward_ref(c)
            P.check_bound(dl, ref["dlogit"], f"{(B, L, G, D, f64)} dlogit")
            P.check_bound_any(dmu, ref["dmu"], "dmu")
            P.check_bound(dls, ref["dlog_sigma"], "dlog_sigma")


@pytest.mark.parametrize("B,S", P.VOTE_COLUMNS)
def test_emulated_vote_finish(B, S):
    for zero_at in (None, (B - 1, 17)):
        c = P.vote_case(B, S, zero_at)
        xyz, feat, inv = P.emulate_vote_finish(c)
        P.check_vote_finish(xyz, feat, inv, P.vote_finish_ref(c), zero_at, f"{(B, S)}")
        f, i = P.vote_grad_inputs(c)
        for wx, wf in ((True, True), (False, True), (True, False)):
            d_net, d_sf = P.emulate_vote_grad(c, f, i, wx, wf)
            P.check_vote_grad(d_net, d_sf, P.vote_grad_ref(c, f, i, wx, wf), zero_at, f"{(B, S)} grad")


def test_emulated_rowsum_and_gather_grad():
    for V in range(1, 65):
        x = P.rowsum_case(257, V)
        P.check_bound(P.emulate_rowsum(x, 1.0 / V), P.rowsum_ref(x, 1.0 / V), f"V {V}")
    for inds in (P.designed_inds_40(), P.designed_inds_130()):
        S = inds.shape[1]
        dout = torch.randn(1, S, 7 * 5, generator=P._gen("gg", S))
        assert torch.equal(P.emulate_gather_grad(dout, inds, 7, 13, 5), P.gather_grad_ref(dout, inds, 7, 13, 5))


def test_nearest_prefix_reference_is_argmin_and_defines_nan():
    cum, target = P.prefix_case(2, 257, 257)
    want = torch.argmin(torch.abs(cum.unsqueeze(-1) - target.unsqueeze(1)), dim=1)
    assert torch.equal(P.nearest_prefix_ref(cum, target), want)
    bad = cum.clone()
    bad[0, 100] = float("nan")                       # an interior NaN never wins, where torch.argmin returns it
    got = P.nearest_prefix_ref(bad, target)
    assert (got[0] != 100).all() and (torch.argmin(torch.abs(bad.unsqueeze(-1) - target.unsqueeze(1)), dim=1)[0] == 100).all()
    assert torch.equal(got[1], want[1])
    bad = cum.clone()
    bad[1, 0] = float("nan")                         # a NaN at frame 0 is never displaced
    assert (P.nearest_prefix_ref(bad, target)[1] == 0).all()


# ---- every mutant is caught, on a named case --------------------------------------------------------------------------------------
def _gemm_hits(mutant, job0=None):
    return [j.name for j in P.GEMM_JOBS if _gemm_rejects(j.name, mutant, job0)]


def _mutant_stale_group():
    hits = _gemm_hits("stale_group")
    assert hits == [j.name for j in P.GEMM_JOBS if P.kpad_of(j.K) // 16 >= 9], hits
    assert {"f144x63", "f192x64", "f208x65", "f560x256", "t547x63"} <= set(hits)
    return hits


def _mutant_kpad_rows_live():
    hits = _gemm_hits("kpad_rows_live")
    assert hits == [j.name for j in P.GEMM_JOBS if j.w_t and j.K % 16], hits
    assert "t15x17" in hits and "t547x63" in hits
    return hits


def _mutant_job0_dims():
    """inside the list of 8, behind f80x16 (k = 80): every job with a larger k loses its rows of T(x) beyond 80"""
    (B, L), names = P.GEMM_LISTS[8]
    job0 = P.GEMM_BY_NAME[names[0]]
    hits = [n for n in names[1:] if _gemm_rejects(n, "job0_dims", job0)]
    assert hits == ["t547x63", "f192x64", "f128x17"], hits
    (B, L), names = P.GEMM_LISTS[2]
    assert _gemm_rejects("f560x256", "job0_dims", P.GEMM_BY_NAME[names[0]])
    return hits


def _mutant_stats_row_clamped():
    hits = _gemm_hits("stats_row_clamped")
    want = [j.name for j in P.GEMM_JOBS if j.stats and j.rows % 16 and (j.bias or j.epi == 1)]
    assert hits == want and {"f64x15", "f128x17", "t15x17", "t17x65"} <= set(hits), (hits, want)
    return hits


def _mutant_gate_on_acc():
    hits = _gemm_hits("gate_on_acc")
    assert hits == [j.name for j in P.GEMM_JOBS if j.epi == 1], hits
    return hits


def _mutant_dead_wave_unwritten():
    hits = _gemm_hits("dead_wave_unwritten")
    assert hits == [j.name for j in P.GEMM_JOBS if j.rows > 256], hits
    assert "f64x257" in hits
    return hits


def _wgrad_hits(mutant):
    hits = set()
    for j in P.WGRAD_JOBS:
        for B, L in P.WGRAD_COLUMNS:
            chunks = B * L // 64
            ops = P.wgrad_operands(j.name, B, L)
            for split in P.wgrad_splits(chunks):
                dw, db = P.emulate_wgrad(j, ops, chunks, split, mutant)
                if _caught(lambda: P.check_wgrad(j, dw, db, P.wgrad_ref(j, ops, chunks, split), chunks, split)):
                    hits.add((j.name, chunks, split))
    return hits


def _mutant_drop_last_chunk():
    hits = _wgrad_hits("drop_last_chunk")
    want = {(j.name, c, s) for j in P.WGRAD_JOBS for c in (1, 3, 4) for s in P.wgrad_splits(c)}
    assert hits == want, want - hits             # every call has a range with a chunk
    return len(hits)


def _mutant_empty_range_unwritten():
    hits = _wgrad_hits("empty_range_unwritten")
    want = {(j.name, c, s) for j in P.WGRAD_JOBS for c in (1, 3, 4) for s in P.wgrad_splits(c)
            if any(lo == hi for lo, hi in P.wgrad_ranges(c, s))}
    assert hits == want and ("w129x129", 3, 4) in hits and ("w1x1", 1, 2) in hits, hits ^ want
    return len(hits)


def _mutant_reduce_drop_tail():
    hits = [(Pn, M) for Pn in P.REDUCE_P for M in P.REDUCE_M
            if _caught(lambda: P.check_bound(P.emulate_reduce(P.reduce_case(Pn, M), "reduce_drop_tail"), P.reduce_ref(P.reduce_case(Pn, M))))]
    assert hits == [(Pn, M) for Pn in (1, 2, 3, 5, 7, 9) for M in P.REDUCE_M], hits
    return hits


def _finalize_hits(mutant, momentum=0.1, kind="plain"):
    return [(Pn, C) for Pn in P.FIN_P for C in P.FIN_C if _caught(lambda: P.check_finalize(
        P.emulate_finalize(P.finalize_case(Pn, C, kind), momentum, mutant=mutant), P.finalize_ref(P.finalize_case(Pn, C, kind), momentum)))]


def _mutant_merge_no_between():
    hits = _finalize_hits("merge_no_between")
    assert hits == [(Pn, C) for Pn in P.FIN_P[1:] for C in P.FIN_C], hits        # a single entry has nothing between
    return hits


def _mutant_biased_running_var():
    hits = _finalize_hits("biased_running_var")
    assert hits == [(Pn, C) for Pn in P.FIN_P for C in P.FIN_C], hits
    assert not _finalize_hits("biased_running_var", momentum=-1.0)               # nothing is written then
    return hits


def _mix_hits(mutant):
    hits = []
    for B, L in P.MIX_COLS:
        for G in P.MIX_G:
            c = P.mix_case(B, L, G, 3, 0)
            pred, pi = P.emulate_mix_forward(c, True, mutant)
            if _caught(lambda: P.check_bound_any(pred, P.mix_forward_ref(c, True))) or _caught(lambda: P.check_bound(pi, P.pi_ref(c))):
                hits.append((B * L, G))
    return hits


def _mutant_mix_cols_16():
    hits = _mix_hits("mix_cols_16")
    assert hits == [(n, G) for n in (1, 15, 17, 111, 257, 600) for G in P.MIX_G], hits
    return hits


def _mutant_mix_slice_16():
    hits = _mix_hits("mix_slice_16")
    assert hits == [(B * L, G) for B, L in P.MIX_COLS for G in (1, 15, 17, 100)], hits
    return hits


def _gather_hits(mutant, T=13):
    hits = []
    for name, inds in (("inds40", P.designed_inds_40()), ("inds130", P.designed_inds_130())):
        S = inds.shape[1]
        dout = torch.randn(1, S, 7 * 5, generator=P._gen("gg", S))
        got, want = P.emulate_gather_grad(dout, inds, 7, T, 5, mutant), P.gather_grad_ref(dout, inds, 7, T, 5)
        if not torch.equal(got, want):
            hits.append((name, sorted(set((got != want).nonzero()[:, 2].tolist()))))
    return hits


def _mutant_hits_overflow():
    hits = _gather_hits("hits_overflow")
    assert hits == [("inds40", [0]), ("inds130", [9])], hits          # the frames with 17 seeds, not the one with 16
    return hits


def _mutant_ragged_frames():
    hits = _gather_hits("ragged_frames")
    assert hits == [("inds40", [8, 9, 10, 11, 12]), ("inds130", [8, 9, 10, 11, 12])], hits
    return hits


def _mutant_rowsum_odd_tail():
    hits = [V for V in range(1, 65) if _caught(
        lambda: P.check_bound(P.emulate_rowsum(P.rowsum_case(257, V), 1.0, "rowsum_odd_tail"), P.rowsum_ref(P.rowsum_case(257, V), 1.0)))]
    assert hits == list(range(1, 65, 2)), hits
    return hits


CATCHERS = {"stale_group": _mutant_stale_group, "kpad_rows_live": _mutant_kpad_rows_live, "job0_dims": _mutant_job0_dims,
            "stats_row_clamped": _mutant_stats_row_clamped, "gate_on_acc": _mutant_gate_on_acc,
            "drop_last_chunk": _mutant_drop_last_chunk, "empty_range_unwritten": _mutant_empty_range_unwritten,
            "reduce_drop_tail": _mutant_reduce_drop_tail, "merge_no_between": _mutant_merge_no_between,
            "biased_running_var": _mutant_biased_running_var, "mix_cols_16": _mutant_mix_cols_16,
            "mix_slice_16": _mutant_mix_slice_16, "hits_overflow": _mutant_hits_overflow, "ragged_frames": _mutant_ragged_frames,
            "rowsum_odd_tail": _mutant_rowsum_odd_tail, "dead_wave_unwritten": _mutant_dead_wave_unwritten}


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_mutant_is_caught(mutant):
    assert set(CATCHERS) == set(P.MUTANTS)
    print(f"MUTANT {mutant} caught: {CATCHERS[mutant]()}")


def test_the_stride_loops_are_checked():
    """entries beyond the first 64 lost in the merges: caught from P = 65 on; columns beyond 256 lost in the mixture
    backward: caught at 257 and 600 columns"""
    hits = _finalize_hits("fin_first_trip")
    assert hits == [(Pn, C) for Pn in (65, 130) for C in P.FIN_C], hits
    for Pn in (65, 130):
        part, fin, M = P.bwd_finalize_case(Pn, 5)
        assert _caught(lambda: P.check_bwd_finalize(P.emulate_bwd_finalize(part, fin, M, 1, "fin_first_trip"),
                                                    P.bwd_finalize_ref(part, fin, M, 1)))
    for B, L in P.MIX_COLS:
        c = P.mix_case(B, L, 17, 2, 1)
        dl, dmu, dls = P.emulate_mix_backward(c, "mix_stride_once")
        ref = P.mix_backward_ref(c)
        bad = _caught(lambda: P.check_bound(dl, ref["dlogit"])) and _caught(lambda: P.check_bound_any(dmu, ref["dmu"])) \
            and _caught(lambda: P.check_bound(dls, ref["dlog_sigma"]))
        assert bad == (B * L > 256), (B, L)


def test_zero_norm_and_closed_gates_are_strict():
    c = P.vote_case(1, 64, (0, 17))
    xyz, feat, inv = P.emulate_vote_finish(c)
    ref = P.vote_finish_ref(c)
    leak = feat.clone()
    leak[0, :, 17] = 0.0                             # a kernel that "repairs" the row is not the reference's division
    with pytest.raises(AssertionError, match="zero-norm"):
        P.check_vote_finish(xyz, leak, inv, ref, (0, 17))
    hurt = feat.clone()
    hurt[0, 3, 18] = float("nan")                    # and a neighbour must not be disturbed
    with pytest.raises(AssertionError, match="NaN"):
        P.check_vote_finish(xyz, hurt, inv, ref, (0, 17))
    j, ops, full, stats = _gemm("t17x65")
    out = P.gemm_out_slice(j, full).clone()
    closed = (~P.gemm_gate(j, ops)).nonzero()[0]
    out[tuple(closed)] = 1e-30
    with pytest.raises(AssertionError):
        P.check_gemm(j, ops, out, None)
    bad = stats.clone()
    bad[0, 0, 0] += 1e-3
    with pytest.raises(AssertionError, match="s1"):
        P.check_gemm(j, ops, P.gemm_out_slice(j, full), bad)


# ---- op level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,S", P.OP_COLUMNS)
@pytest.mark.parametrize("kind", P.OP_KINDS)
def test_op_cases_band_share(kind, B, S, train):
    """at most BAND_CAP of the float64 chain's ReLU gates lie within their layer's own bound of zero"""
    ref = P.op_ref(kind, B, S, train)
    assert len(ref["bands"]) == (11 if kind == "proposal_heads" else 2)
    for name, b in ref["bands"].items():
        print(f"{kind} {(B, S)} train {train} {name}: {b['count']} of {b['n']} gates inside the band")
        assert b["share"] <= P.BAND_CAP, name
        assert (b["dbeta"] >= 0).all() and b["dbeta"].shape == b["dgamma"].shape
    assert all(torch.isfinite(v).all() for v in ref["param"].values())


def test_op_ref_is_the_plain_module_chain():
    """the hooks that record the gates change nothing, and the check accepts the fp32 chain while rejecting a lost term"""
    ref = P.op_ref("vote_head", 3, 64, True)
    mod = P.op_module("vote_head").double().train(True)
    inp = P.op_inputs("vote_head", 3, 64)
    x = inp["feats"].double().requires_grad_(True)
    net = mod.conv_input(x.transpose(1, 2))
    (net * inp["g_net"].double()).sum().backward()
    assert torch.equal(net.detach(), ref["out"]["net"]) and torch.equal(x.grad, ref["grad"]["dx"])
    for n, p in mod.named_parameters():
        assert torch.equal(p.grad, ref["param"][n]), n
    assert int(ref["buffer"]["conv_input.0.batchnorm.num_batches_tracked"]) == 1
    two = P.op_ref("vote_head", 1, 64, True, momentum_none=True, calls=2)
    assert int(two["buffer"]["conv_input.1.batchnorm.num_batches_tracked"]) == 2
    f32 = P.op_module("vote_head").train(True)
    xf = inp["feats"].clone().requires_grad_(True)
    nf = f32.conv_input(xf.transpose(1, 2))
    (nf * inp["g_net"]).sum().backward()
    got = {"out": {"net": nf.detach()}, "grad": {"dx": xf.grad}, "param": {n: p.grad for n, p in f32.named_parameters()},
           "buffer": {n: b.detach() for n, b in f32.named_buffers()}}
    print(P.op_check("vote_head", got, ref))
    got["param"]["conv_input.1.batchnorm.bias"] = got["param"]["conv_input.1.batchnorm.bias"].clone()
    got["param"]["conv_input.1.batchnorm.bias"][7] *= 1.01
    with pytest.raises(AssertionError, match="conv_input.1.batchnorm.bias"):
        P.op_check("vote_head", got, ref)

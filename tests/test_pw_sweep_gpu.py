"""GPU: the point-wise head kernels (csrc/pw_layers.hip, p2rnet/pw_op.py) and the seams of the backbone
(csrc/seed_ops.hip, p2rnet/seed_op.py) against the float64 references of tests/pw_cases.py.

Stage level, through the C entry points on poison-filled outputs inside poisoned halos (halos intact, no element left
unwritten, everything outside a job's slice still poison): p2r_pw_gemm over the designed job list of pw_cases.GEMM_JOBS
(every K of both weight layouts, every row count, the NLC input and output paths with each of their scalar triggers,
transforms, epilogues, slices) and job lists of 2, 5 and 8, each job bit-identical to the same job launched alone;
p2r_pw_wgrad + p2r_pw_reduce over rows, K in {1, 63, 64, 65, 129}, the four layout pairs, every split incl. one with an
empty range, job lists of 3 and 8; p2r_pw_reduce alone incl. 48 jobs in one launch; p2r_pw_bn_finalize /
p2r_pw_bn_bwd_finalize across the 64-lane stride with unequal counts, |mean| / std = 1000, a constant channel, job lists
into one `fin` / `coef`, evaluation mode, four momenta, the step counter given / NULL; p2r_mdn_mix_forward / backward
over ragged 16-column workgroups, G around 16, D 1..4, f32 and f64, four mixed heads in one launch, rows inside a wider
logit tensor; the seams at their partition edges (ragged 8-frame chunks, hit counts 0, 1, 2, 3, 16, 17, hits of one frame
from three ballot trips, out-of-range indices, a zero-norm vote row, NaN in nearest_prefix); every refusal (-22, nothing
written) and the empty calls.  Every stage is evaluated on the kernel's OWN fp32 inputs under the derived running-error
bounds; the comparison functions are the ones tests/test_pw_reference_cpu.py proves sensitive.

Op level, through pw_op.vote_head, pw_op.votes_normalized and pw_op.proposal_heads: outputs, running statistics, the step
counter and every gradient against the module chain in FLOAT64 (not the fp32 chain on the same device), train and eval,
at (B, columns) = (1, 64), (3, 64), (2, 128), with the tolerances of tests/test_pw_gpu.py; a ReLU gate within its layer's
rounding band of zero moves a whole term between per-channel sums, so each parameter gradient gets the slack of its
undecided terms on top of the tolerance and nothing is masked out; momentum=None over two calls (pw_op._momentum reads the
step counter on the host); S = 96, where `*_supported` is false, through the public module.

Worst observed error / derived bound per stage (one run on an MI355X; 1 would be at the limit):
  pw_gemm epilogue 0 (31 jobs + 3 lists): out 0.18, tile mean 0.32, tile M2 0.21;  epilogue 1 (15): out 0.19, s1 0.24, s2 0.18
  pw_wgrad (11 jobs x 3 column counts x 3-4 splits): dw 0.11, db 0.14; pw_reduce of those partials 0.60 / 0.54, alone (40) 0.50
  pw_bn_finalize (180 calls): constants 0.98 (one rounding: half an ulp reaches the bound), running mean 0.66, variance 0.64
  pw_bn_bwd_finalize (60): coef 0.68, dgamma 0.96, dbeta 0.97 (one rounding)
  mdn_mix (7 column counts x 5 G x 8 heads): f32 pred 0.11, pi 0.18, dlogit 0.21, dmu 0.16, dlog_sigma 0.15;
                                              f64 pred 0.16, pi 0.17, dlogit 0.21, dmu 0.15, dlog_sigma 0.13
  expf: max |pi - float64 sigmoid| = 2.153 ulps of pi over the sweep's 1.2 million logits (pw_cases.PI_ULP_MEASURED), so
        pw_cases.EXPF_ULP = max(2, ceil(2 x 2.153)) = 5 is what the mixture bounds allow for expf
  rowsum_short (256 calls) 0.46;  vote_finish feat 0.37, inv_norm 0.26, vote_finish_grad 0.79
  gather_frames, gather_frames_grad, nearest_prefix: bit for bit
Op level, worst error / borrowed tolerance over (1, 64), (3, 64), (2, 128) x train / eval; 241 of the float64 chains' 2.5
million gates lay inside their layer's band, none of them cost a comparison its tolerance:
  vote_head: net (1e-5) 0.075, dx (2e-4) 0.0035, parameter gradients (2e-4) 0.0040, running statistics (1e-5) 0.015
  votes_normalized: xyz (1e-5) 0.035, features (1e-5) 0.061, d seed_xyz (1e-6) 0 (exact), dx 0.0038, parameters 0.0043
  proposal_heads: center / size / heading / sem_obj (2e-5) 0.016 / 0.016 / 0.012 / 0.026, dx (2e-4) 0.0026,
                  parameter gradients (3e-4) 0.0032, running statistics (1e-5) 0.016
  momentum=None, two calls: running statistics 0.027 (vote head), 0.045 (proposal heads)
so the borrowed tolerances have a headroom of 13 (vote_head's output) to 300 (parameter gradients), the derived stage
bounds at most 5 -- and none where a stage is a single rounding.
"""
import pytest
import torch

from tests import memguard
from tests import pw_cases as P

pytestmark = pytest.mark.gpu

EINVAL = "failed with status -22"
F32, F64 = torch.float32, torch.float64


def _out(shape, dev, dtype=F32, offset_bytes=0):
    return memguard.guarded(shape, dtype, dev, fill="poison", halo="poison", offset_bytes=offset_bytes)


def _in(t, dev, offset_bytes=0):
    return memguard.guarded(t.shape, t.dtype, dev, fill=t, halo="zero", offset_bytes=offset_bytes)[1]


def _kept(fill, dev):
    """an in/out buffer (running statistics, step counter) inside a poisoned halo"""
    return memguard.guarded(fill.shape, fill.dtype, dev, fill=fill, halo="poison")


def _halo_ok(*pairs):
    for buf, view in pairs:
        assert int(memguard.halo_damage(buf, view, "poison")) == 0, "written outside the buffer"


def _written(*pairs):
    torch.cuda.synchronize()
    res = []
    for p in pairs:
        if p is None:
            res.append(None)
            continue
        _halo_ok(p)
        assert int(memguard.poison_count(p[1])) == 0, "an element was never written"
        res.append(p[1].cpu())
    return res


def _untouched(*pairs):
    torch.cuda.synchronize()
    for buf, view in pairs:
        _halo_ok((buf, view))
        assert int(memguard.poison_count(view)) == view.numel(), "written although the call does nothing"


def _refused(name, call, outs):
    with pytest.raises(RuntimeError, match=name + " " + EINVAL):
        call()
    _untouched(*outs)


def _pw():
    from pose2room_amd.p2rnet import pw_op
    return pw_op


def _stream(dev):
    from pose2room_amd import _lib
    return _lib.current_stream(dev)


def _launch(dev, name, *args):
    from pose2room_amd import _lib
    _lib.launch(name, dev, *args)


def _ratios(stage, ratios):
    print(f"RATIO {stage} " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


# ---- p2r_pw_gemm ----------------------------------------------------------------------------------------------------------------
def _gemm_job(dev, j, B, L, keep):
    """-> (job dict, out pair, stats pair or None); the device operands are appended to `keep`"""
    at = _pw()._at
    ops = P.gemm_operands(j.name, B, L)
    d = {k: _in(v, dev) for k, v in ops.items()}
    keep.append(d)
    out = _out(P.gemm_out_shape(j, B, L), dev)
    stats = _out((B * L // 64, j.rows, 3 if j.epi == 0 else 2), dev) if j.stats else None
    job = dict(x=at(d["x"], j.xc0 if j.x_nlc else j.xc0 * L), w=at(d["w"]), out=at(out[1], j.oc0 if j.out_nlc else j.oc0 * L),
               stats=at(stats[1]) if stats else None, k=j.K, rows=j.rows, x_ctot=j.K + j.xs, x_nlc=j.x_nlc, w_t=j.w_t,
               out_ctot=j.rows + j.os, out_nlc=j.out_nlc, epilogue=j.epi, bias=at(d.get("bias")))
    if j.tr:
        job.update(tr=at(d["tr"]), tr_mode=j.tr, tr_ld=j.K + j.ld)
    if j.tr == 2:
        job["x2"] = at(d["x2"], j.xc0 if j.x_nlc else j.xc0 * L)
    if j.epi == 1:
        job.update(mz=at(d["mz"], j.mc0 * L), mz_ctot=j.rows + j.ms, mfin=at(d["mfin"]), mfin_ld=j.rows + j.ld)
    return job, out, stats


def _gemm_result(j, out, stats, B, L):
    """halos intact, the job's slice written, everything else still poison -> (full output, stats) on the CPU"""
    torch.cuda.synchronize()
    _halo_ok(out)
    full = out[1].cpu()
    assert int(memguard.poison_count(P.gemm_out_slice(j, full).contiguous())) == 0, f"{j.name}: an element was never written"
    assert int(memguard.poison_count(full)) == full.numel() - j.rows * B * L, f"{j.name}: written outside the job's channels"
    return full, (_written(stats)[0] if stats else None)


_SINGLE = {}


def _gemm_alone(dev, name, B, L):
    if (name, B, L) not in _SINGLE:
        j = P.GEMM_BY_NAME[name]
        keep = []
        job, out, stats = _gemm_job(dev, j, B, L, keep)
        _pw()._gemm([job], B, L, _stream(dev))
        _SINGLE[name, B, L] = _gemm_result(j, out, stats, B, L)
    return _SINGLE[name, B, L]


@pytest.mark.parametrize("name", [j.name for j in P.GEMM_JOBS])
def test_pw_gemm(dev, name):
    j = P.GEMM_BY_NAME[name]
    B, L = P.gemm_columns(j)
    full, stats = _gemm_alone(dev, name, B, L)
    _ratios("pw_gemm" + str(j.epi), P.check_gemm(j, P.gemm_operands(name, B, L), P.gemm_out_slice(j, full), stats))


@pytest.mark.parametrize("n", sorted(P.GEMM_LISTS))
def test_pw_gemm_job_list(dev, n):
    """jobs of different k, rows, layout and epilogue in one launch: the LDS tile is sized by the largest kpad, the job is
    picked by blockIdx.x / colblocks; every job's output and statistics are the bits of the same job launched alone"""
    (B, L), names = P.GEMM_LISTS[n]
    keep, built = [], []
    for name in names:
        built.append(_gemm_job(dev, P.GEMM_BY_NAME[name], B, L, keep))
    _pw()._gemm([b[0] for b in built], B, L, _stream(dev))
    for name, (_, out, stats) in zip(names, built):
        j = P.GEMM_BY_NAME[name]
        full, st = _gemm_result(j, out, stats, B, L)
        alone, st_alone = _gemm_alone(dev, name, B, L)
        assert memguard.same_bits(full, alone), f"{name}: differs from the single launch"
        assert st is None or memguard.same_bits(st, st_alone), f"{name}: statistics differ from the single launch"
        _ratios("pw_gemm" + str(j.epi), P.check_gemm(j, P.gemm_operands(name, B, L), P.gemm_out_slice(j, full), st))


def test_pw_gemm_refusals_and_empty_batch(dev):
    at, st = _pw()._at, _stream(dev)
    B, L = 1, 64
    x, x2, w = (torch.randn(600 * 64 + 4, device=dev) for _ in range(3))
    tr = torch.randn(3 * 600, device=dev)
    out = _out((1, 64, 64), dev)

    def job(**kw):
        base = dict(x=at(x), w=at(w), out=at(out[1]), k=64, rows=64, x_ctot=64, out_ctot=64)
        base.update(kw)
        return base
    call = lambda jobs, Bn=B, Ln=L: (lambda: _pw()._gemm(jobs, Bn, Ln, st))
    cases_ = {"9 jobs": call([job() for _ in range(9)]), "L % 64": call([job()], 1, 96), "K 561": call([job(k=561, x_ctot=561, w_t=1)]),
              "row-major K % 16": call([job(k=24, x_ctot=24)]), "x off 16": call([job(x=at(x, 1))]), "w off 16": call([job(w=at(w, 1))]),
              "x2 off 16": call([job(x2=at(x2, 1), tr=at(tr), tr_mode=2, tr_ld=64)]), "tr_mode 1 no tr": call([job(tr_mode=1, tr_ld=64)]),
              "tr_mode 2 no tr": call([job(x2=at(x2), tr_mode=2, tr_ld=64)]), "tr_mode 2 no x2": call([job(tr=at(tr), tr_mode=2, tr_ld=64)]),
              "epilogue 1 no mz": call([job(epilogue=1, mfin=at(tr), mfin_ld=64)]),
              "epilogue 1 no mfin": call([job(epilogue=1, mz=at(x2), mz_ctot=64)]), "epilogue 2": call([job(epilogue=2, mz=at(x2), mfin=at(tr))]),
              "k 0": call([job(k=0)]), "rows 0": call([job(rows=0)]), "no out": call([job(out=None)])}
    for what, c in cases_.items():
        _refused("p2r_pw_gemm", c, [out])
    _pw()._gemm([job()], 0, 64, st)                   # B = 0: OK, nothing written
    _untouched(out)
    _pw()._gemm([job(k=560, x_ctot=560, w_t=1)], B, L, st)          # and the largest K is accepted
    _written(out)


# ---- p2r_pw_wgrad, p2r_pw_reduce ---------------------------------------------------------------------------------------------------
def _wgrad_job(dev, j, B, L, split, keep):
    at = _pw()._at
    ops = P.wgrad_operands(j.name, B, L)
    d = {k: _in(v, dev) for k, v in ops.items()}
    keep.append(d)
    dw = _out((split, j.rows, j.K), dev)
    db = _out((split, j.rows), dev) if j.db else None
    job = dict(x=at(d["x"], j.xc0 if j.x_nlc else j.xc0 * L), x_nlc=j.x_nlc, x_ctot=j.rows + j.xs, rows=j.rows,
               y=at(d["y"], j.yc0 if j.y_nlc else j.yc0 * L), y_nlc=j.y_nlc, y_ctot=j.K + j.ys, k=j.K, dw_part=at(dw[1]),
               db_part=at(db[1]) if db else None, split=split)
    if j.tr == 2:
        job.update(x2=at(d["x2"], j.xc0 if j.x_nlc else j.xc0 * L), tr=at(d["tr"]), tr_mode=2, tr_ld=j.rows + j.ld)
    if j.ytr:
        job.update(ytr=at(d["ytr"]), ytr_ld=j.K + j.ld)
    return job, dw, db


def _reduce_call(dev, pairs):
    """pairs: [(partials on the device [P, ...], M)] -> outputs on the CPU, one launch"""
    outs = [_out((M,), dev) for _, M in pairs]
    _pw()._reduce([(p, o[1]) for (p, _), o in zip(pairs, outs)], _stream(dev))
    return _written(*outs)


@pytest.mark.parametrize("name", [j.name for j in P.WGRAD_JOBS])
def test_pw_wgrad_and_reduce(dev, name):
    j = P.WGRAD_BY_NAME[name]
    worst = {}
    for B, L in P.WGRAD_COLUMNS:
        chunks = B * L // 64
        ops = P.wgrad_operands(name, B, L)
        for split in P.wgrad_splits(chunks):
            keep = []
            job, dw, db = _wgrad_job(dev, j, B, L, split, keep)
            _pw()._wgrad([job], B, L, _stream(dev))
            dwc, dbc = _written(dw, db)
            ratios = P.check_wgrad(j, dwc, dbc, P.wgrad_ref(j, ops, chunks, split), chunks, split, f"{name} {(B, L)} split {split}")
            pairs = [(dw[1], j.rows * j.K)] + ([(db[1], j.rows)] if db else [])
            for key, part, red in zip(("dw_sum", "db_sum"), (dwc, dbc), _reduce_call(dev, pairs)):
                ratios[key] = P.check_bound(red, P.reduce_ref(part.reshape(split, -1)), f"{name} split {split} {key}")
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    _ratios("pw_wgrad", worst)


@pytest.mark.parametrize("n", sorted(P.WGRAD_LISTS))
def test_pw_wgrad_job_list(dev, n):
    """jobs with different tile counts and splits behind one blk0[] table, each bit-identical to a launch of its own"""
    (B, L), entries = P.WGRAD_LISTS[n]
    keep, built = [], []
    for name, split in entries:
        built.append(_wgrad_job(dev, P.WGRAD_BY_NAME[name], B, L, split, keep))
    _pw()._wgrad([b[0] for b in built], B, L, _stream(dev))
    for (name, split), (_, dw, db) in zip(entries, built):
        j = P.WGRAD_BY_NAME[name]
        job, dw1, db1 = _wgrad_job(dev, j, B, L, split, keep)
        _pw()._wgrad([job], B, L, _stream(dev))
        (a, b), (a1, b1) = _written(dw, db), _written(dw1, db1)
        assert memguard.same_bits(a, a1) and (b is None or memguard.same_bits(b, b1)), f"{name}: differs from the single launch"
        P.check_wgrad(j, a, b, P.wgrad_ref(j, P.wgrad_operands(name, B, L), B * L // 64, split), B * L // 64, split)


def test_pw_reduce(dev):
    """every P % 4 and M around the 256-thread workgroup; all 40 jobs in one launch, then 48, then 49 refused"""
    combos = [(Pn, M) for Pn in P.REDUCE_P for M in P.REDUCE_M]
    ins = [P.reduce_case(Pn, M) for Pn, M in combos]
    dins = [t.to(dev) for t in ins]
    got = _reduce_call(dev, [(d, M) for d, (_, M) in zip(dins, combos)])
    worst = 0.0
    for (Pn, M), inp, g in zip(combos, ins, got):
        worst = max(worst, P.check_bound(g, P.reduce_ref(inp), f"P {Pn} M {M}"))
    _ratios("pw_reduce", {"out": worst})
    got48 = _reduce_call(dev, [(d, M) for d, (_, M) in zip((dins + dins)[:48], (combos + combos)[:48])])
    for a, b in zip(got48, (got + got)[:48]):
        assert memguard.same_bits(a, b)
    at = _pw()._at
    outs = [_out((M,), dev) for _, M in (combos + combos)[:49]]
    jobs = [dict(in_=at(d), out=at(o[1]), P=Pn, M=M) for d, (Pn, M), o in zip((dins + dins)[:49], (combos + combos)[:49], outs)]
    call = lambda js: (lambda: _pw()._launch("p2r_pw_reduce", _pw()._RJob, js, _stream(dev)))
    _refused("p2r_pw_reduce", call(jobs), outs)
    for bad in (dict(P=0), dict(M=0), dict(in_=None), dict(out=None)):
        _refused("p2r_pw_reduce", call([{**jobs[0], **bad}]), outs[:1])


# ---- p2r_pw_bn_finalize, p2r_pw_bn_bwd_finalize ----------------------------------------------------------------------------------
def _bn_job(dev, case, momentum, fin, off, fin_ld, nbt, evalmode=False, keep=None):
    at = _pw()._at
    d = {k: case[k].to(dev) for k in ("part", "gamma", "beta")}
    run = [_kept(case[k], dev) for k in ("running_mean", "running_var")]
    keep.append((d, run))
    Pn, C = case["part"].shape[:2]
    job = dict(part=None if evalmode else at(d["part"]), gamma=at(d["gamma"]), beta=at(d["beta"]), running_mean=at(run[0][1]),
               running_var=at(run[1][1]), fin=at(fin[1], off), num_batches_tracked=at(nbt[1]) if nbt else None, eps=P.EPS,
               momentum=momentum, P=0 if evalmode else Pn, C=C, fin_ld=fin_ld)
    return job, run


def _bn_launch(dev, jobs):
    _pw()._launch("p2r_pw_bn_finalize", _pw()._BnJob, jobs, _stream(dev))


@pytest.mark.parametrize("kind", P.FIN_KINDS)
@pytest.mark.parametrize("Pn", P.FIN_P)
def test_pw_bn_finalize(dev, Pn, kind):
    worst = {}
    for C in P.FIN_C:
        case = P.finalize_case(Pn, C, kind)
        for i, momentum in enumerate(P.FIN_MOMENTUM):
            with_nbt = (i + Pn) % 2 == 0
            keep = []
            fin = _out((4, C), dev)
            nbt = _kept(torch.tensor([5]), dev)
            job, run = _bn_job(dev, case, momentum, fin, 0, C, nbt if with_nbt else None, keep=keep)
            _bn_launch(dev, [job])
            out, rm, rv, steps = _written(fin, run[0], run[1], nbt)
            label = f"P {Pn} C {C} {kind} momentum {momentum}"
            assert steps.item() == (6 if with_nbt and momentum >= 0 else 5), label
            ratios = P.check_finalize({"out": out, "running_mean": rm, "running_var": rv}, P.finalize_ref(case, momentum), label)
            if momentum <= 0:           # 0: the update keeps the old value exactly; < 0: nothing is written
                assert memguard.same_bits(rm, case["running_mean"]) and memguard.same_bits(rv, case["running_var"]), label
            if momentum == 1.0:
                assert memguard.same_bits(rm, out[0]), label
            if kind == "const":
                assert out[1, 0] == torch.tensor(1.0 / P.EPS ** 0.5, dtype=F64).float() and out[0, 0] == 0.7109375, label
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    _ratios("pw_bn_finalize", worst)


def test_pw_bn_finalize_job_list_and_eval(dev):
    """three jobs of different C and P with channel offsets into one fin (fin_ld = 112 > C); the columns of fin outside
    every job's channels stay poison; then evaluation mode: the running buffers and the counter do not change"""
    layout = [(5, 65, 2), (1, 130, 9), (96, 63, 12)]             # (C, P, first column)
    fin_ld = 112
    for evalmode in (False, True):
        keep, jobs, runs, nbts = [], [], [], []
        fin = _out((4, fin_ld), dev)
        for C, Pn, off in layout:
            nbt = _kept(torch.tensor([7]), dev)
            job, run = _bn_job(dev, P.finalize_case(Pn, C), -1.0 if evalmode else 0.1, fin, off, fin_ld, nbt, evalmode, keep)
            jobs.append(job), runs.append(run), nbts.append(nbt)
        _bn_launch(dev, jobs)
        torch.cuda.synchronize()
        _halo_ok(fin)
        full = fin[1].cpu()
        used = torch.zeros(fin_ld, dtype=torch.bool)
        for (C, Pn, off), run, nbt in zip(layout, runs, nbts):
            used[off:off + C] = True
            case = P.finalize_case(Pn, C)
            rm, rv, steps = _written(run[0], run[1], nbt)
            got = {"out": full[:, off:off + C].contiguous(), "running_mean": rm, "running_var": rv}
            if evalmode:
                ones = torch.ones(C, dtype=F64)
                ref = P.bn_cases._finalize_from(case["running_mean"].double(), case["running_var"].double(), ones, case, -1.0, P.EPS)
                assert steps.item() == 7 and memguard.same_bits(rm, case["running_mean"]) and memguard.same_bits(rv, case["running_var"])
            else:
                ref = P.finalize_ref(case, 0.1)
                assert steps.item() == 8
            P.check_finalize(got, ref, f"list C {C} eval {evalmode}")
        assert int(memguard.poison_count(full[:, ~used].contiguous())) == 4 * int((~used).sum()), "fin written outside the jobs' channels"
        assert int(memguard.poison_count(full[:, used].contiguous())) == 0


@pytest.mark.parametrize("Pn", P.FIN_P)
def test_pw_bn_bwd_finalize(dev, Pn):
    """train 0 / 1, dgamma / dbeta given / NULL, and the three C as one job list with offsets into one coef / fin"""
    at = _pw()._at
    offs, ld = {1: 3, 5: 6, 96: 14}, 112
    call = lambda jobs: _pw()._launch("p2r_pw_bn_bwd_finalize", _pw()._BnbJob, jobs, _stream(dev))
    worst = {}
    for train in (1, 0):
        for with_grads in (True, False):
            fin_all = torch.full((4, ld), P.NAN)
            for C in P.FIN_C:
                fin_all[:, offs[C]:offs[C] + C] = P.bwd_finalize_case(Pn, C)[1]
            dfin, coef = fin_all.to(dev), _out((3, ld), dev)
            jobs, outs, parts = [], [], []
            for C in P.FIN_C:
                part, fin, M = P.bwd_finalize_case(Pn, C)
                parts.append(part.to(dev))
                dg, db = (_out((C,), dev), _out((C,), dev)) if with_grads else (None, None)
                outs.append((dg, db))
                jobs.append(dict(part=at(parts[-1]), fin=at(dfin, offs[C]), coef=at(coef[1], offs[C]), dgamma=at(dg[1]) if dg else None,
                                 dbeta=at(db[1]) if db else None, M=M, P=Pn, C=C, fin_ld=ld, coef_ld=ld, train=train))
            call(jobs)
            torch.cuda.synchronize()
            _halo_ok(coef)
            full = coef[1].cpu()
            used = torch.zeros(ld, dtype=torch.bool)
            for C, (dg, db) in zip(P.FIN_C, outs):
                used[offs[C]:offs[C] + C] = True
                part, fin, M = P.bwd_finalize_case(Pn, C)
                got = {"coef": full[:, offs[C]:offs[C] + C].contiguous()}
                if with_grads:
                    got["dgamma"], got["dbeta"] = _written(dg, db)
                for k, v in P.check_bwd_finalize(got, P.bwd_finalize_ref(part, fin, M, train), f"P {Pn} C {C} train {train}").items():
                    worst[k] = max(worst.get(k, 0.0), v)
                if not train:
                    assert not got["coef"][1:].any()
            assert int(memguard.poison_count(full)) == 3 * int((~used).sum()), "coef written outside the jobs' channels"
    _ratios("pw_bn_bwd_finalize", worst)


def test_pw_bn_refusals(dev):
    at = _pw()._at
    case = P.finalize_case(1, 5)
    d = {k: v.to(dev) for k, v in case.items() if k != "M"}
    fin, coef = _out((4, 5), dev), _out((3, 5), dev)
    base = dict(part=at(d["part"]), gamma=at(d["gamma"]), beta=at(d["beta"]), running_mean=at(d["running_mean"]),
                running_var=at(d["running_var"]), fin=at(fin[1]), num_batches_tracked=None, eps=P.EPS, momentum=0.1, P=1, C=5, fin_ld=5)
    call = lambda js: (lambda: _bn_launch(dev, js))
    for bad in (dict(C=0), dict(P=0), dict(gamma=None), dict(beta=None), dict(fin=None), dict(running_mean=None),
                dict(part=None, P=0, running_var=None)):
        _refused("p2r_pw_bn_finalize", call([{**base, **bad}]), [fin])
    _refused("p2r_pw_bn_finalize", call([base] * 9), [fin])
    assert torch.equal(d["running_mean"].cpu(), case["running_mean"])
    bbase = dict(part=at(d["part"]), fin=at(d["part"]), coef=at(coef[1]), dgamma=None, dbeta=None, M=64.0, P=1, C=5, fin_ld=5, coef_ld=5, train=1)
    bcall = lambda js: (lambda: _pw()._launch("p2r_pw_bn_bwd_finalize", _pw()._BnbJob, js, _stream(dev)))
    for bad in (dict(C=0), dict(P=0), dict(part=None), dict(fin=None), dict(coef=None), dict(M=0.0)):
        _refused("p2r_pw_bn_bwd_finalize", bcall([{**bbase, **bad}]), [coef])
    _refused("p2r_pw_bn_bwd_finalize", bcall([bbase] * 9), [coef])


# ---- p2r_mdn_mix_forward, p2r_mdn_mix_backward ------------------------------------------------------------------------------------
def _mix_heads(dev, cs, specs, with_pi, keep):
    """-> (forward head dicts, backward head dicts, outputs per head)"""
    at = _pw()._at
    fwd, bwd, outs = [], [], []
    for c, h in zip(cs, specs):
        d = {k: c[k].to(dev) for k in ("logit", "mu", "log_sigma", "eps", "dpred")}
        keep.append(d)
        B, ctot, L = c["logit"].shape
        G, D = c["mu"].shape
        dt = c["mu"].dtype
        o = {"pred": _out((B, L, D), dev, dt), "pi": _out((B, G, L), dev) if with_pi else None, "dlogit": _out((B, ctot, L), dev),
             "dmu": _out((G, D), dev, dt), "dls": _out((G, D), dev)}
        common = dict(logit=at(d["logit"], c["c0"] * L), log_sigma=at(d["log_sigma"]), mu=at(d["mu"]), eps=at(d["eps"]) if h.eps else None,
                      D=D, f64=h.f64)
        fwd.append(dict(common, pred=at(o["pred"][1]), pi=at(o["pi"][1]) if with_pi else None))
        bwd.append(dict(common, eps=at(d["eps"]), dpred=at(d["dpred"]), dlogit=at(o["dlogit"][1], c["c0"] * L), dmu=at(o["dmu"][1]),
                        dlog_sigma=at(o["dls"][1])))
        outs.append(o)
    return fwd, bwd, outs


def _mix_call(dev, name, heads, *dims):
    MH = _pw()._MixHead
    arr = (MH * len(heads))(*[MH(**h) for h in heads])
    _launch(dev, name, len(heads), arr, *dims)


def _mix_collect(c, o, with_pi):
    G, c0 = c["G"], c["c0"]
    pred, dmu, dls = _written(o["pred"], o["dmu"], o["dls"])
    pi = _written(o["pi"])[0] if with_pi else None
    torch.cuda.synchronize()
    _halo_ok(o["dlogit"])
    dl_full = o["dlogit"][1].cpu()
    dl = dl_full[:, c0:c0 + G].contiguous()
    assert int(memguard.poison_count(dl)) == 0 and int(memguard.poison_count(dl_full)) == dl_full.numel() - dl.numel(), \
        "dlogit: the head's rows are not exactly what was written"
    return {"pred": pred, "pi": pi, "dlogit": dl, "dmu": dmu, "dls": dls}


@pytest.mark.parametrize("B,L", P.MIX_COLS)
def test_mdn_mix(dev, B, L):
    """four heads of mixed D / type / noise in one launch, each bit-identical to the same head alone; G around the 16
    slices; at G = 17 the heads' rows sit in the middle of wider logit / dlogit tensors"""
    worst, ulps = {}, 0.0
    for G, launch in [(G, launch) for G in P.MIX_G for launch in P.MIX_LAUNCHES]:
        extra, c0 = (7, 3) if G == 17 else (0, 0)
        cs = [P.mix_case(B, L, G, h.D, h.f64, extra, c0) for h in launch]
        keep = []
        fwd, bwd, outs = _mix_heads(dev, cs, launch, True, keep)
        _mix_call(dev, "p2r_mdn_mix_forward", fwd, B, G, L, G + extra)
        _mix_call(dev, "p2r_mdn_mix_backward", bwd, B, G, L, G + extra, G + extra)
        for i, (c, h, o) in enumerate(zip(cs, launch, outs)):
            got = _mix_collect(c, o, True)
            f1, b1, o1 = _mix_heads(dev, [c], [h], False, keep)          # alone, and without the pi output
            _mix_call(dev, "p2r_mdn_mix_forward", f1, B, G, L, G + extra)
            _mix_call(dev, "p2r_mdn_mix_backward", b1, B, G, L, G + extra, G + extra)
            alone = _mix_collect(c, o1[0], False)
            for k in ("pred", "dlogit", "dmu", "dls"):
                assert memguard.same_bits(got[k], alone[k]), f"head {i} G {G}: {k} differs from the single launch"
            label = f"{(B, L)} G {G} D {h.D} f64 {h.f64}"
            ref = P.mix_backward_ref(c)
            r = {"pred": P.check_bound_any(got["pred"], P.mix_forward_ref(c, bool(h.eps)), label + " pred"),
                 "pi": P.check_bound(got["pi"], P.pi_ref(c), label + " pi"),
                 "dlogit": P.check_bound(got["dlogit"], ref["dlogit"], label + " dlogit"),
                 "dmu": P.check_bound_any(got["dmu"], ref["dmu"], label + " dmu"),
                 "dls": P.check_bound(got["dls"], ref["dlog_sigma"], label + " dlog_sigma")}
            assert got["pred"].dtype == c["mu"].dtype and got["dmu"].dtype == c["mu"].dtype
            ulps = max(ulps, P.pi_ulps(got["pi"], c))
            for k, v in r.items():
                key = k + ("_f64" if h.f64 else "")
                worst[key] = max(worst.get(key, 0.0), v)
    _ratios("mdn_mix", worst)
    print(f"RATIO expf pi_ulps {ulps:.4f}")
    assert ulps <= P.EXPF_ULP


def test_mdn_mix_refusals_and_empty_batch(dev):
    B, L, G = 1, 17, 15
    c = P.mix_case(B, L, G, 3, 0)
    keep = []
    fwd, bwd, outs = _mix_heads(dev, [c], [P.MixHead(3, 0, 1)], True, keep)
    o = outs[0]
    fouts, bouts = [o["pred"], o["pi"]], [o["dlogit"], o["dmu"], o["dls"]]
    fcall = lambda heads, Bn=B: (lambda: _mix_call(dev, "p2r_mdn_mix_forward", heads, Bn, G, L, G))
    bcall = lambda heads, Bn=B: (lambda: _mix_call(dev, "p2r_mdn_mix_backward", heads, Bn, G, L, G, G))
    for bad in (dict(D=0), dict(D=5), dict(mu=None), dict(pred=None), dict(logit=None), dict(log_sigma=None)):
        _refused("p2r_mdn_mix_forward", fcall([{**fwd[0], **bad}]), fouts)
    _refused("p2r_mdn_mix_forward", fcall(fwd * 5), fouts)
    for bad in (dict(D=0), dict(D=5), dict(mu=None), dict(dpred=None), dict(log_sigma=None), dict(dlogit=None), dict(dmu=None),
                dict(dlog_sigma=None)):
        _refused("p2r_mdn_mix_backward", bcall([{**bwd[0], **bad}]), bouts)
    _refused("p2r_mdn_mix_backward", bcall(bwd * 5), bouts)
    # B = 0: the forward is an empty call (OK, nothing written); the backward refuses, since dmu / dlog_sigma would have to
    # be written as zeros by a launch of no columns (include/p2r_hip.h says so)
    fcall(fwd, 0)()
    _untouched(*fouts)
    _refused("p2r_mdn_mix_backward", bcall(bwd, 0), bouts)


# ---- the seams: p2r_gather_frames, p2r_gather_frames_grad ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,J", P.GATHER_CJ)
def test_gather_frames(dev, C, J):
    """C J around the 256-thread stride; indices -1 and T among valid ones give zero rows with the neighbours intact"""
    Bn, T, S = 2, 9, 7
    x = torch.randn(Bn, C, T, J, generator=P._gen("gather", C, J))
    inds = torch.tensor([[0, 8, -1, 3, 9, 3, 8], [9, -1, 0, 0, 4, -7, 8]])
    out = _out((Bn, S, C * J), dev)
    _launch(dev, "p2r_gather_frames", Bn, C, T, J, S, x.to(dev), inds.to(dev), out[1])
    got, = _written(out)
    assert torch.equal(got, P.gather_ref(x, inds))
    assert not got[0, 2].any() and not got[0, 4].any() and not got[1, 5].any() and got[0, 3].any()
    for b, s in ((0, S), (Bn, 0)):
        out = _out((Bn, S, C * J), dev)
        _launch(dev, "p2r_gather_frames", b, C, T, J, s, x.to(dev), inds.to(dev), out[1])
        _untouched(out)
    for bad in ((-1, C, T, J, S), (Bn, 0, T, J, S), (Bn, C, 0, J, S), (Bn, C, T, 0, S), (Bn, C, T, J, -1)):
        _refused("p2r_gather_frames", lambda: _launch(dev, "p2r_gather_frames", *bad, x.to(dev), inds.to(dev), out[1]), [out])


def _gather_grad(dev, dout, inds, C, T, J):
    Bn, S = inds.shape
    dx = _out((Bn, C, T, J), dev)
    _launch(dev, "p2r_gather_frames_grad", Bn, C, T, J, S, dout.to(dev), inds.to(dev), dx[1])
    return _written(dx)[0]


@pytest.mark.parametrize("T", P.GRAD_T)
def test_gather_frames_grad_shapes(dev, T):
    """ragged last chunk of 8 frames (T % 8), the eight-channel unroll and its tail (C), J around one; random picks with
    duplicates and out-of-range indices; S = 0 writes zeros"""
    for C in P.GRAD_C:
        for J in P.GRAD_J:
            S = 11
            g = P._gen("ggrad", T, C, J)
            inds = torch.randint(-1, T + 1, (2, S), generator=g)
            dout = torch.randn(2, S, C * J, generator=g)
            got = _gather_grad(dev, dout, inds, C, T, J)
            assert torch.equal(got, P.gather_grad_ref(dout, inds, C, T, J)), (T, C, J)
            picked = P.hit_counts(inds, T) > 0
            assert not got.permute(0, 2, 1, 3)[~picked].any()
    zero = _gather_grad(dev, torch.zeros(2, 1, 7 * 5), torch.zeros(2, 0, dtype=torch.int64), 7, T, 5)
    assert zero.shape == (2, 7, T, 5) and not zero.any() and not torch.signbit(zero).any()


@pytest.mark.parametrize("which", ["inds40", "inds130"])
def test_gather_frames_grad_hit_counts(dev, which):
    """inds40: frames picked 17, 16, 3, 2, 1, 0 times and frame 12 once in the ragged chunk: the three branches <= 2,
    <= GF_MAXHIT, > GF_MAXHIT at their boundaries.  inds130: the seeds {0, 63, 64, 65, 129} of one frame come from three
    ballot trips, another frame is picked 17 times across the trips, indices -1 and T contribute nothing.  Rows are added
    in ascending seed order: a sequential fp32 loop is the reference, bit for bit, and so is a second call."""
    inds = P.designed_inds_40() if which == "inds40" else P.designed_inds_130()
    S = inds.shape[1]
    for C, J in ((9, 5), (8, 53), (1, 1)):
        dout = torch.randn(1, S, C * J, generator=P._gen("gg", S, C, J))
        got = _gather_grad(dev, dout, inds, C, 13, J)
        want = P.gather_grad_ref(dout, inds, C, 13, J)
        assert torch.equal(got, want), (C, J, sorted(set((got != want).nonzero()[:, 2].tolist())))
        assert memguard.same_bits(got, _gather_grad(dev, dout, inds, C, 13, J))
        unpicked = P.hit_counts(inds, 13)[0] == 0
        assert unpicked.any() and not got[0][:, unpicked].any()
    dx = _out((1, 9, 13, 5), dev)
    for bad in ((-1, 9, 13, 5, S), (1, 0, 13, 5, S), (1, 9, 0, 5, S), (1, 9, 13, 0, S), (1, 9, 13, 5, -1)):
        _refused("p2r_gather_frames_grad", lambda: _launch(dev, "p2r_gather_frames_grad", *bad, dout.to(dev), inds.to(dev), dx[1]), [dx])
    _launch(dev, "p2r_gather_frames_grad", 0, 9, 13, 5, S, dout.to(dev), inds.to(dev), dx[1])
    _untouched(dx)


# ---- p2r_rowsum_short, p2r_vote_finish, p2r_vote_finish_grad, p2r_nearest_prefix ----------------------------------------------------
@pytest.mark.parametrize("rows", P.ROWSUM_ROWS)
def test_rowsum_short(dev, rows):
    worst = 0.0
    for V in range(1, 65):
        x = P.rowsum_case(rows, V)
        scale = 1.0 / V if V % 2 else 1.0
        out = _out((rows,), dev)
        _launch(dev, "p2r_rowsum_short", rows, V, scale, x.to(dev), out[1])
        got, = _written(out)
        worst = max(worst, P.check_bound(got, P.rowsum_ref(x, float(torch.tensor(scale, dtype=F32))), f"rows {rows} V {V}"))
    _ratios("rowsum_short", {"out": worst})
    out = _out((rows,), dev)
    x = torch.zeros(rows, 65, device=dev)
    for r, V in ((rows, 0), (rows, 65), (-1, 5)):
        _refused("p2r_rowsum_short", lambda: _launch(dev, "p2r_rowsum_short", r, V, 1.0, x, out[1]), [out])
    _launch(dev, "p2r_rowsum_short", 0, 5, 1.0, x, out[1])
    _untouched(out)


@pytest.mark.parametrize("B,S", P.VOTE_COLUMNS)
def test_vote_finish_and_grad(dev, B, S):
    worst = {}
    for zero_at in (None, (B - 1, 17)):
        c = P.vote_case(B, S, zero_at)
        d = {k: v.to(dev) for k, v in c.items()}
        xyz, feat, inv = _out((B, S, 3), dev), _out((B, P.VF_C, S), dev), _out((B, S), dev)
        _launch(dev, "p2r_vote_finish", B, S, P.VF_C, d["net"], d["sf"], d["hip"], xyz[1], feat[1], inv[1])
        torch.cuda.synchronize()
        _halo_ok(xyz, feat, inv)
        got = [t[1].cpu() for t in (xyz, feat, inv)]
        assert all(int(memguard.poison_count(t)) == 0 for t in got)
        r = P.check_vote_finish(*got, P.vote_finish_ref(c), zero_at, f"{(B, S)} zero {zero_at}")
        for wx, wf in ((True, True), (False, True), (True, False)):
            d_net, d_sf = _out((B, S, 3 + P.VF_C), dev), _out((B, S, P.VF_C), dev)
            _launch(dev, "p2r_vote_finish_grad", B, S, P.VF_C, d["d_xyz"] if wx else None, d["d_feat"] if wf else None, feat[1], inv[1],
                    d_net[1], d_sf[1])
            torch.cuda.synchronize()
            _halo_ok(d_net, d_sf)
            gn, gs = d_net[1].cpu(), d_sf[1].cpu()
            assert int(memguard.poison_count(gn)) == 0 and int(memguard.poison_count(gs)) == 0
            r["df"] = max(r.get("df", 0.0), P.check_vote_grad(gn, gs, P.vote_grad_ref(c, got[1], got[2], wx, wf), zero_at,
                                                               f"{(B, S)} grad xyz {wx} feat {wf}")["df"])
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _ratios("vote_finish", worst)
    fresh = [_out((B, S, 3), dev), _out((B, P.VF_C, S), dev), _out((B, S), dev)]
    gfresh = [_out((B, S, 3 + P.VF_C), dev), _out((B, S, P.VF_C), dev)]
    for b, s, C in ((B, 96, 256), (B, S, 128), (B, 0, 256), (-1, S, 256)):
        _refused("p2r_vote_finish", lambda: _launch(dev, "p2r_vote_finish", b, s, C, d["net"], d["sf"], d["hip"],
                                                    *[f[1] for f in fresh]), fresh)
        _refused("p2r_vote_finish_grad", lambda: _launch(dev, "p2r_vote_finish_grad", b, s, C, d["d_xyz"], d["d_feat"], feat[1], inv[1],
                                                         *[f[1] for f in gfresh]), gfresh)
    _launch(dev, "p2r_vote_finish", 0, S, P.VF_C, d["net"], d["sf"], d["hip"], *[f[1] for f in fresh])
    _launch(dev, "p2r_vote_finish_grad", 0, S, P.VF_C, d["d_xyz"], d["d_feat"], feat[1], inv[1], *[f[1] for f in gfresh])
    _untouched(*fresh, *gfresh)


@pytest.mark.parametrize("T", P.PREFIX_T)
def test_nearest_prefix(dev, T):
    """T across the 256-thread staging loop and the 64 KB of LDS a kernel may use by default; S off a multiple of 256;
    plateaus and targets exactly midway"""
    for S in P.PREFIX_S:
        Bn = 2 if T < 1000 else 1
        cum, target = P.prefix_case(Bn, T, S)
        out = _out((Bn, S), dev, torch.int64)
        _launch(dev, "p2r_nearest_prefix", Bn, T, S, cum.to(dev), target.to(dev), out[1])
        got, = _written(out)
        assert torch.equal(got, P.nearest_prefix_ref(cum, target)), (T, S)
        if T <= 257:
            assert torch.equal(got, torch.argmin(torch.abs(cum.unsqueeze(-1) - target.unsqueeze(1)), dim=1))


def test_nearest_prefix_nan_refusals_and_the_op(dev):
    """a NaN at an interior frame never wins (torch.argmin would return it); a NaN at frame 0 is never displaced: index 0.
    The model's arc lengths are a cumulative sum starting at 0 with targets derived from its last entry: a NaN there makes
    every distance NaN and both rules give index 0, a valid frame."""
    from pose2room_amd.p2rnet import seed_op
    cum, target = P.prefix_case(2, 257, 255)
    interior, first = cum.clone(), cum.clone()
    interior[0, 100], first[1, 0] = P.NAN, P.NAN
    for c in (interior, first):
        got = seed_op.nearest_prefix(c.to(dev), target.to(dev)).cpu()
        assert torch.equal(got, P.nearest_prefix_ref(c, target))
    assert (seed_op.nearest_prefix(interior.to(dev), target.to(dev)).cpu()[0] != 100).all()
    assert (seed_op.nearest_prefix(first.to(dev), target.to(dev)).cpu()[1] == 0).all()
    allnan = torch.full_like(target, P.NAN)
    assert not seed_op.nearest_prefix(interior.to(dev), allnan.to(dev)).any()
    out = _out((1, 4), dev, torch.int64)
    big = torch.zeros(1, 40001, device=dev)
    for b, t, s in ((1, 40001, 4), (1, 0, 4), (-1, 5, 4), (1, 5, -1)):
        _refused("p2r_nearest_prefix", lambda: _launch(dev, "p2r_nearest_prefix", b, t, s, big, big, out[1]), [out])
    for b, s in ((0, 4), (1, 0)):
        _launch(dev, "p2r_nearest_prefix", b, 5, s, big, big, out[1])
        _untouched(out)


def test_wgrad_refusals_and_empty_batch(dev):
    at, st = _pw()._at, _stream(dev)
    x, y, tr = torch.randn(64 * 64 + 4, device=dev), torch.randn(64 * 64 + 4, device=dev), torch.randn(3 * 64, device=dev)
    dw = _out((1, 64, 64), dev)
    base = dict(x=at(x), x_ctot=64, rows=64, y=at(y), y_ctot=64, k=64, dw_part=at(dw[1]), split=1)
    call = lambda js, Bn=1, Ln=64: (lambda: _pw()._wgrad(js, Bn, Ln, st))
    for bad in (dict(rows=0), dict(k=0), dict(split=0), dict(x=None), dict(y=None), dict(dw_part=None), dict(tr_mode=1, tr=at(tr)),
                dict(tr_mode=2, tr=at(tr)), dict(tr_mode=2, x2=at(y)), dict(x=at(x, 1)), dict(y=at(y, 1)),
                dict(tr_mode=2, tr=at(tr), x2=at(y, 1))):
        _refused("p2r_pw_wgrad", call([{**base, **bad}]), [dw])
    _refused("p2r_pw_wgrad", call([dict(base) for _ in range(9)]), [dw])
    _refused("p2r_pw_wgrad", call([dict(base)], 1, 96), [dw])
    call([dict(base)], 0, 64)()
    _untouched(dw)


# ---- op level: pw_op.vote_head, pw_op.votes_normalized, pw_op.proposal_heads against the float64 module chain ----------------------
def _run_op(dev, kind, B, S, train, momentum_none=False, calls=1):
    """the fused op on the device, `calls` consecutive forward / backward passes -> the dict layout of pw_cases.op_ref"""
    pw_op = _pw()
    mod = P.op_module(kind).to(dev).train(train)
    if momentum_none:
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.momentum = None
    for call in range(calls):
        mod.zero_grad()
        inp = {k: v.to(dev) for k, v in P.op_inputs(kind, B, S, call).items()}
        feats = inp["feats"].clone().requires_grad_(True)
        grads = {}
        if kind == "proposal_heads":
            assert pw_op.proposal_heads_supported(mod, feats)
            eps = {k: inp["eps_" + k] for k in ("center", "size", "heading")}
            pc, ps, ph, sem = pw_op.proposal_heads(mod, feats, eps)
            outs = {"center": pc, "size": ps, "heading": ph, "sem": sem}
            sum((outs[k] * inp["g_" + k]).sum().double() for k in outs).backward()
        elif kind == "vote_head":
            assert pw_op.vote_head_supported(mod, feats)
            outs = {"net": pw_op.vote_head(mod, feats)}
            (outs["net"] * inp["g_net"]).sum().backward()
        else:
            xyz_in = inp["seed_xyz"].clone().requires_grad_(True)
            assert pw_op.votes_normalized_supported(mod, xyz_in, feats)
            xyz, f = pw_op.votes_normalized(mod, xyz_in, feats)
            assert f.transpose(1, 2).is_contiguous()
            outs = {"xyz": xyz, "feat": f}
            ((xyz * inp["g_xyz"]).sum() + (f.transpose(1, 2) * inp["g_feat"]).sum()).backward()
            grads["dxyz"] = xyz_in.grad.cpu()
        grads["dx"] = feats.grad.cpu()
    torch.cuda.synchronize()
    return {"out": {k: v.detach().cpu() for k, v in outs.items()}, "grad": grads,
            "param": {n: p.grad.cpu() for n, p in mod.named_parameters() if p.grad is not None},
            "buffer": {n: b.detach().cpu() for n, b in mod.named_buffers()}}


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,S", P.OP_COLUMNS)
@pytest.mark.parametrize("kind", P.OP_KINDS)
def test_heads_against_the_float64_module_chain(dev, kind, B, S, train):
    ref = P.op_ref(kind, B, S, train)
    got = _run_op(dev, kind, B, S, train)
    und = sum(b["count"] for b in ref["bands"].values())
    print(f"{kind} {(B, S)} train {train}: {und} gates of the float64 chain inside their layer's band")
    _ratios("op_" + kind, P.op_check(kind, got, ref, f"{kind} {(B, S)} train {train}"))
    if not train:
        start = {n: b for n, b in P.op_module(kind).named_buffers()}
        assert all(torch.equal(got["buffer"][n], start[n]) for n in start), "evaluation mode changed a buffer"


def test_heads_cumulative_average(dev):
    """momentum=None, two consecutive training calls: the running statistics follow torch's cumulative average 1 / (step + 1).
    pw_op._momentum reads num_batches_tracked on the host (a device-to-host copy per BatchNorm and call)."""
    for kind in ("vote_head", "proposal_heads"):
        ref = P.op_ref(kind, 1, 64, True, momentum_none=True, calls=2)
        got = _run_op(dev, kind, 1, 64, True, momentum_none=True, calls=2)
        steps = [int(v) for n, v in got["buffer"].items() if n.endswith("num_batches_tracked") and n in _stepped(kind)]
        assert steps and all(s == 2 for s in steps), steps
        _ratios("op_cumulative_" + kind, P.op_check(kind, got, ref, kind + " momentum None"))


def _stepped(kind):
    """the step counters of the BatchNorm layers the op runs through"""
    mod = P.op_module(kind)
    names = {n for n, _ in mod.named_buffers() if n.endswith("num_batches_tracked")}
    if kind == "proposal_heads":
        return {n for n in names if n.split(".")[0] in ("conv_center", "conv_size", "conv_heading", "conv_sem_obj", "gmm_center",
                                                        "gmm_size", "gmm_heading")}
    return names


def test_unsupported_shape_takes_the_module_chain(dev):
    """S = 96 is no multiple of 64: `vote_head_supported` / `proposal_heads_supported` are false and the public module must
    give the module chain's result, bit for bit (it IS the module chain then)"""
    from pose2room_amd.p2rnet.modules import vote_center
    pw_op = _pw()
    S = P.OP_FALLBACK_S
    inp = {k: v.to(dev) for k, v in P.op_inputs("votes_normalized", 2, S).items()}
    res = []
    for fused in (True, False):
        mod = P.op_module("votes_normalized").to(dev).train(True)
        feats = inp["feats"].clone().requires_grad_(True)
        assert not pw_op.vote_head_supported(mod, feats) and not pw_op.votes_normalized_supported(mod, inp["seed_xyz"], feats)
        vote_center.USE_FUSED_HEAD = fused
        try:
            xyz, f = mod(inp["seed_xyz"], feats)
        finally:
            vote_center.USE_FUSED_HEAD = True
        ((xyz * inp["g_xyz"]).sum() + (f.transpose(1, 2) * inp["g_feat"]).sum()).backward()
        res.append([xyz, f, feats.grad] + [p.grad for p in mod.parameters()] + [b for b in mod.buffers()])
    assert all(memguard.same_bits(a, b) for a, b in zip(*res))
    chain = P.op_module("vote_head").double()
    want = chain.conv_input(inp["feats"].cpu().double().transpose(1, 2)).transpose(1, 2).detach()
    assert float((res[0][0].detach().cpu() - (inp["seed_xyz"].cpu()[:, :, chain.origin_joint_id] + want[..., :3])).abs().max()) < 1e-4
    det = P.op_module("proposal_heads").to(dev)
    assert not pw_op.proposal_heads_supported(det, torch.zeros(2, 256, S, device=dev))

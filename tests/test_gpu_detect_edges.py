"""-m gpu: the detector's box, loss and RoIAlign kernels (csrc/rpn_kernels.hip, csrc/detect_kernels.hip) at their edges -- the
tables, float64 references and measured bounds of tests/detect_edge_cases.py; test_detect_edge_cases_host.py pins those on the CPU.

A  test_rpn_loss / test_fastrcnn_loss      saturated logits, residuals on and next to beta, every label pattern, num_sampled apart
                                           from the label count, past the 1024-block grid; exact zeros, finite, reproducible
B  test_box_decode_* / test_encode_decode  the dw / dh clamp, zero width, boxes outside the clip rectangle, the second grid trip
C  test_anchor_match_* / test_nms*         IoUs exactly on hi, lo and the NMS threshold, tied ground truths and anchors, zero-area
                                           boxes, padding behind the counts, past 256 blocks: EVERY element equals the oracle
D  test_roi_align* / test_ml_*             samples on -1, 0, H - 1, H and one float32 step outside; zero-size aligned RoIs; images
                                           with 0 .. 300 RoIs; every grid trip; C up to 1024; the refusals; adjointness
E  test_mask_targets_*                     averages of exactly 0.5

Lines printed:  DETEDGE <case> dloss=..u24 dgrad/bound=.. e_ref=..u24   (B, D: the error over its bound in place of dloss / dgrad)"""
import ctypes as C

import numpy as np
import pytest

import detect_edge_cases as D
from oracle import detection_ref
from rfi_toolbox_amd._lib import RfiHipError, check, lib
from rfi_toolbox_amd.models import detection_ops as ops

pytestmark = pytest.mark.gpu
F32, F64, U24 = np.float32, np.float64, D.U24


def _ctx():
    from rfi_toolbox_amd.runtime import Context
    return Context.get(0)


def _P(d):
    return C.c_void_p(d.ptr)


def _same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _u24(err, scale):
    return err / (U24 * max(scale, 1e-300))


# ------------------------------------------------------------------------------------------------------------ A
def _check_loss(name, got, again, want, e_ref):
    (l1, l2, g), (w1, w2, g64) = got, want
    d1, d2 = abs(l1 - w1), abs(l2 - w2)
    dgrad = float(np.abs(g.astype(F64) - g64).max()) if np.isfinite(g).all() else float("inf")
    bound = D.grad_bound(e_ref, g64)
    gmax = float(np.abs(g64).max())
    print(f"DETEDGE {name} dloss={max(_u24(d1, max(1.0, abs(w1))), _u24(d2, max(1.0, abs(w2)))):.2f}u24 "
          f"dgrad/bound={dgrad / bound if bound > 0 else dgrad:.2f} e_ref={_u24(e_ref, gmax) if gmax > 0 else 0.0:.2f}u24 "
          f"dgrad={_u24(dgrad, gmax) if gmax > 0 else dgrad:.2f}u24")
    assert np.isfinite(g).all() and np.isfinite([l1, l2]).all()
    assert d1 <= D.loss_bound(w1) and d2 <= D.loss_bound(w2), (l1, w1, l2, w2)
    assert dgrad <= bound, (dgrad, bound, e_ref)
    assert _same_bits((F32(l1), F32(l2), g), (F32(again[0]), F32(again[1]), again[2]))


@pytest.mark.parametrize("case", D.RPN_CASES, ids=lambda c: c.id)
def test_rpn_loss(case):
    head, lab, tg, ns, _, _ = D.rpn_inputs(case)
    want, e_ref, _ = D.loss_figures(D.rpn_ref, head, lab, tg, case.A, case.beta, ns)
    got = ops.rpn_loss(head, lab, tg, case.A, beta=case.beta, num_sampled=ns)
    again = ops.rpn_loss(head, lab, tg, case.A, beta=case.beta, num_sampled=ns)
    _check_loss("rpn_" + case.id, got, again, want, e_ref)
    g = got[2]
    obj, box = g[:, :case.A].reshape(-1), g[:, case.A:].reshape(-1, 4)
    assert (obj[lab < 0] == 0).all() and not np.signbit(obj[lab < 0]).any()        # exactly +0.0 for the anchors not sampled
    assert (box[lab <= 0] == 0).all()                                               # no box gradient but for the positives


@pytest.mark.parametrize("case", D.FRC_CASES, ids=lambda c: c.id)
def test_fastrcnn_loss(case):
    head, lab, tg, _, _ = D.frc_inputs(case)
    want, e_ref, _ = D.loss_figures(D.frc_ref, head, lab, tg, case.beta)
    got = ops.fastrcnn_loss(head, lab, tg, beta=case.beta)
    again = ops.fastrcnn_loss(head, lab, tg, beta=case.beta)
    _check_loss("frc_" + case.id, got, again, want, e_ref)
    box = got[2][:, case.K1:].reshape(case.R, case.K1, 4)
    other = np.arange(case.K1)[None, :] != lab[:, None]
    assert (box[other] == 0).all() and (box[lab == 0] == 0).all()                   # only the label's own deltas, never a background row's


# ------------------------------------------------------------------------------------------------------------ B
def _check_decode(name, got, anchors, deltas, clip):
    want = detection_ref.decode_boxes(anchors, deltas, clip)
    steps = D.decode_steps(anchors, deltas)
    e_ref = float((np.abs(D.decode32(anchors, deltas, clip) - want) / steps).max())
    err = float((np.abs(got.astype(F64) - want) / steps).max())
    bound = D.decode_bound(e_ref)
    print(f"DETEDGE {name} derr/bound={err / bound:.2f} e_ref={e_ref:.2f}steps derr={err:.2f}steps")
    assert np.isfinite(got).all() and err <= bound, (err, bound)
    return bound, steps


@pytest.mark.parametrize("clip", [None, D.CLIP], ids=["unclipped", "clipped"])
def test_box_decode_table(clip):
    d = D.decode_deltas()
    got = ops.decode_boxes(D.DECODE_ANCHORS, d, image_size=clip)
    bound, steps = _check_decode(f"decode_table_{'clipped' if clip else 'unclipped'}", got, D.DECODE_ANCHORS, d, clip)
    assert got.tobytes() == ops.decode_boxes(D.DECODE_ANCHORS, d, image_size=clip).tobytes()
    if clip:
        free = detection_ref.decode_boxes(D.DECODE_ANCHORS, d)
        lim = np.array([clip[1], clip[0], clip[1], clip[0]], F32)[None, :]
        assert (got >= 0).all() and (got <= lim).all()                              # in [0, clip] exactly
        over, under = free > lim + bound * steps, free < -bound * steps
        assert over.any() and under.any()
        assert np.array_equal(got[over], np.broadcast_to(lim, got.shape)[over])     # on the bound, bit for bit
        assert (got[under] == 0).all() and not np.signbit(got[under]).any()


def test_box_decode_second_trip():
    d = D.decode_large_deltas()
    got = ops.decode_boxes(D.DECODE_ANCHORS, d)
    rows = D.DECODE_LARGE_ROWS
    _check_decode("decode_large_rows", got[rows], D.DECODE_ANCHORS[rows % len(D.DECODE_ANCHORS)], d[rows], None)
    _check_decode("decode_large_all", got, D.DECODE_ANCHORS, d, None)               # (the oracle is vectorised: every row as well)


def test_encode_decode_round_trip():
    a, g = D.roundtrip_boxes()
    lab, mi, t = ops.anchor_match(a, g, 0.7, 0.3)
    assert (lab == 1).all() and np.array_equal(mi, np.arange(len(a)))
    back = ops.decode_boxes(a, t)
    steps = D.decode_steps(a, t)
    e_ref = float((np.abs(D.decode32(a, D.encode32(a, g)) - g.astype(F64)) / steps).max())
    err = float((np.abs(back.astype(F64) - g.astype(F64)) / steps).max())
    print(f"DETEDGE decode_roundtrip derr/bound={err / D.decode_bound(e_ref):.2f} e_ref={e_ref:.2f}steps derr={err:.2f}steps")
    assert err <= D.decode_bound(e_ref)


# ------------------------------------------------------------------------------------------------------------ C
def _match_device(ctx, anchors, ac, gt, gc, hi, lo, lq):
    """rfi_op_anchor_match_batched on the arrays as they are (the rows behind the counts included); outputs pre-filled"""
    shared = anchors.ndim == 2
    B, n = len(gc), anchors.shape[-2]
    da, dg, dgc = ctx.to_device(np.ascontiguousarray(anchors, F32)), ctx.to_device(np.ascontiguousarray(gt, F32)), ctx.to_device(gc)
    dac = None if ac is None else ctx.to_device(ac)
    labels, matched = ctx.to_device(np.full((B, n), 99, np.int8)), ctx.to_device(np.full((B, n), 99, np.int32))
    targets, best = ctx.to_device(np.full((B, n, 4), np.nan, F32)), ctx.empty((B, gt.shape[1]), F32)
    check(lib.rfi_op_anchor_match_batched(ctx.handle, _P(da), n, 0 if shared else n, None if dac is None else _P(dac), _P(dg), B, gt.shape[1],
                                          _P(dgc), float(hi), float(lo), 1 if lq else 0, _P(best), _P(labels), _P(matched), _P(targets)))
    ctx.synchronize()
    return labels.numpy(), matched.numpy(), targets.numpy()


def _check_match(got, anchors, gt, hi, lo, lq, tag):
    """labels and matched indices equal the oracle's EVERYWHERE; targets exactly 0 off the positives and within 4 x 2^-24 max(1,
    |t|) on them (one rounded quotient, or a rounded quotient under a logarithm: each well inside 2 x 2^-24 max(1, |t|))"""
    lab, mi, t = D.ref_anchor_match(anchors, gt, hi, lo, lq)
    assert np.array_equal(got[0], lab), (tag, np.flatnonzero(got[0] != lab)[:8])
    assert np.array_equal(got[1], mi), (tag, np.flatnonzero(got[1] != mi)[:8])
    assert (got[2][lab != 1] == 0).all() and np.isfinite(got[2]).all(), tag
    assert (np.abs(got[2].astype(F64) - t) <= 4 * U24 * np.maximum(1.0, np.abs(t))).all(), tag
    return int((lab == 1).sum())


@pytest.mark.parametrize("hi,lo,lq", D.MATCH_SETTINGS, ids=lambda v: str(v))
def test_anchor_match_ties(hi, lo, lq):
    ctx = _ctx()
    anchors, ac, gt, gc, names = D.match_batch()
    lab, mi, t = _match_device(ctx, anchors, ac, gt, gc, hi, lo, lq)
    again = _match_device(ctx, anchors, ac, gt, gc, hi, lo, lq)
    assert _same_bits((lab, mi, t), again)
    for i, k in enumerate(names):
        _check_match((lab[i, :ac[i]], mi[i, :ac[i]], t[i, :ac[i]]), anchors[i, :ac[i]], gt[i, :gc[i]], hi, lo, lq, k)
        assert (lab[i, ac[i]:] == -2).all() and (mi[i, ac[i]:] == -1).all() and (t[i, ac[i]:] == 0).all(), k      # behind anchor_count
    # the zero-area rule, spelled out: no IoU -> label 0, matched -1, zero targets
    z = names.index("zero_area_only")
    assert (lab[z, :ac[z]] == 0).all() and (mi[z, :ac[z]] == -1).all() and (t[z] == 0).all()
    print(f"DETEDGE match_ties_{hi}_{lo}_{int(lq)} images={len(names)} mismatches=0")


@pytest.mark.parametrize("hi,lo,lq", D.MATCH_SETTINGS[:3], ids=lambda v: str(v))
def test_anchor_match_past_256_blocks(hi, lo, lq):
    """65,836 shared anchors (the second grid trip) and two images: the whole ground-truth list, and none"""
    anchors, gt = D.match_large_anchors(), np.asarray(D.MATCH_LARGE_GT, F32)
    lab, mi, t = ops.anchor_match_batched(anchors, [gt, np.zeros((0, 4), F32)], hi, lo, lq)
    npos = _check_match((lab[0], mi[0], t[0]), anchors, gt, hi, lo, lq, "large")
    assert npos >= 4 and (lab[0][65536:] == 1).any() and len(set(lab[0])) == 3
    assert (lab[1] == 0).all() and (mi[1] == -1).all() and (t[1] == 0).all()                 # G = 0
    print(f"DETEDGE match_large_{hi}_{lo}_{int(lq)} n={len(anchors)} positives={npos} mismatches=0")


@pytest.mark.parametrize("thr", D.THRESHOLDS)
@pytest.mark.parametrize("n", D.NMS_SIZES)
def test_nms_ties(n, thr):
    b = D.nms_boxes(n, thr)
    scores = -np.arange(n, dtype=F32)
    keep = ops.nms(b, scores, thr)
    assert np.array_equal(keep, D.ref_nms(b, thr)) and np.array_equal(keep, ops.nms(b, scores, thr))
    print(f"DETEDGE nms_n{n}_thr{thr} kept={len(keep)} mismatches=0")


@pytest.mark.parametrize("thr", D.THRESHOLDS)
def test_nms_batched_ties(thr):
    boxes, counts = D.nms_batched_sets(thr)
    keep = ops.nms_batched(boxes, counts, thr)
    want = np.zeros(keep.shape, bool)
    for i, c in enumerate(counts):
        want[i, D.ref_nms(boxes[i, :c], thr)] = True
    assert np.array_equal(keep, want) and np.array_equal(keep, ops.nms_batched(boxes, counts, thr))
    print(f"DETEDGE nms_batched_thr{thr} sets={len(counts)} kept={int(keep.sum())} mismatches=0")


# ------------------------------------------------------------------------------------------------------------ D
def _fwd(case, x, rois):
    return ops.roi_align(x, rois, case.scale, (case.PH, case.PW), case.sr, case.aligned)


def _bwd(case, dout, shape, rois):
    return ops.roi_align_backward(dout, shape, rois, case.scale, case.sr, case.aligned)


def _check_roi(name, x, dout, got, gotb, want, wantb, e_f, e_b):
    bf, bb = D.roi_bound(e_f, want), D.roi_bound(e_b, wantb)
    df, db = float(np.abs(got.astype(F64) - want).max()), float(np.abs(gotb.astype(F64) - wantb).max())
    lhs, rhs = float((got.astype(F64) * dout).sum()), float((gotb.astype(F64) * x).sum())
    slack = bf * float(np.abs(dout).sum()) + bb * float(np.abs(x).sum())
    print(f"DETEDGE {name} dfwd/bound={df / bf if bf else df:.2f} dbwd/bound={db / bb if bb else db:.2f} "
          f"e_ref={_u24(e_f, np.abs(want).max()) if bf else 0:.2f}/{_u24(e_b, np.abs(wantb).max()) if bb else 0:.2f}u24 "
          f"adjoint={abs(lhs - rhs):.2e} (allowed {slack:.2e})")
    assert np.isfinite(got).all() and np.isfinite(gotb).all()
    assert df <= bf, (df, bf)
    assert db <= bb, (db, bb)
    assert abs(lhs - rhs) <= slack, (lhs, rhs)          # <forward(x), dout> = <x, backward(dout)> within the two bounds


@pytest.mark.parametrize("case", D.ROI_CASES, ids=lambda c: c.id)
def test_roi_align_both_ways(case):
    x, rois, dout = D.roi_inputs(case)
    a = (case.scale, (case.PH, case.PW), case.sr, case.aligned)
    want, wantb = detection_ref.roi_align(x, rois, *a), detection_ref.roi_align_backward(dout, x.shape, rois, *a)
    e_f = float(np.abs(D.roi_align_np(x, rois, *a, f=F32) - want).max())
    e_b = float(np.abs(D.roi_align_bwd_np(dout, x.shape, rois, case.scale, case.sr, case.aligned, F32) - wantb).max())
    got, gotb = _fwd(case, x, rois), _bwd(case, dout, x.shape, rois)
    assert got.tobytes() == _fwd(case, x, rois).tobytes() and gotb.tobytes() == _bwd(case, dout, x.shape, rois).tobytes()
    _check_roi(case.id, x, dout, got, gotb, want, wantb, e_f, e_b)
    if case.kind == "boundary":                      # a sample one step outside [-1, L] gives nothing, one on -1 or L the border pixel
        _, pts = D.boundary_rois(case.H, case.W, case.scale, case.aligned)
        outside = (pts[:, 0] < -1) | (pts[:, 0] > case.H) | (pts[:, 1] < -1) | (pts[:, 1] > case.W)
        assert outside.any() and (got[outside] == 0).all() and (np.abs(got[~outside]).reshape((~outside).sum(), -1).max(1) > 0).all()


def test_roi_align_forward_second_trip():
    case = D.ROI_FWD_TRIP
    x, rois, _ = D.roi_inputs(case)
    a = (case.scale, (case.PH, case.PW), case.sr, case.aligned)
    got = _fwd(case, x, rois)
    rows = list(D.ROI_FWD_TRIP_ROWS)
    want_rows = detection_ref.roi_align(x, rois[rows], *a)                       # the loops on the named rows of both trips ...
    want, r32 = D.roi_align_np(x, rois, *a, f=F64), D.roi_align_np(x, rois, *a, f=F32)       # ... their restatement everywhere
    e_ref = float(np.abs(r32 - want).max())
    bound = D.roi_bound(e_ref, want)
    d_rows, d_all = float(np.abs(got[rows] - want_rows).max()), float(np.abs(got - want).max())
    print(f"DETEDGE {case.id} dfwd/bound={max(d_rows, d_all) / bound:.2f} e_ref={_u24(e_ref, np.abs(want).max()):.2f}u24")
    assert d_rows <= bound and d_all <= bound and got.tobytes() == _fwd(case, x, rois).tobytes()


def test_roi_align_backward_second_trip():
    case = D.ROI_BWD_TRIP
    x, rois, dout = D.roi_inputs(case)
    gotb = _bwd(case, dout, x.shape, rois)
    wantb = detection_ref.roi_align_backward(dout, x.shape, rois, case.scale, (case.PH, case.PW), case.sr, case.aligned)
    e_ref = float(np.abs(D.roi_align_bwd_np(dout, x.shape, rois, case.scale, case.sr, case.aligned, F32) - wantb).max())
    bound = D.roi_bound(e_ref, wantb)
    db = float(np.abs(gotb - wantb).max())
    first = 4096 * 256 // (case.C // 4) // case.W + 1                              # map rows wholly in the second trip
    print(f"DETEDGE {case.id} dbwd/bound={db / bound:.2f} e_ref={_u24(e_ref, np.abs(wantb).max()):.2f}u24")
    assert np.abs(wantb[:, first:]).max() > 0 and db <= bound
    assert gotb.tobytes() == _bwd(case, dout, x.shape, rois).tobytes()


def test_roi_align_backward_without_rois_writes_zeros():
    ctx = _ctx()
    N, H, W, Cc = 2, 5, 9, 4
    dx = ctx.to_device(np.full((N, H, W, Cc), 7.0, F32))                          # stale contents
    dummy = ctx.to_device(np.zeros((1, 8), F32))
    check(lib.rfi_op_roi_align_backward(ctx.handle, _P(dummy), N, H, W, Cc, _P(dummy), 0, 0.5, 2, 2, 2, 0, _P(dx)))
    ctx.synchronize()
    assert (dx.numpy() == 0).all()


def _ml_forward(ctx, case, feats, rois, lv, count):
    df = [ctx.to_device(f) for f in feats]
    maps = (C.c_void_p * 4)(*[f.ptr for f in df])
    R, P_ = len(rois), case.P
    dr, dl, dc = ctx.to_device(rois), ctx.to_device(lv), ctx.to_device(np.array([count, 0], np.int32))
    out = ctx.to_device(np.full((R, P_, P_, case.C), 7.0, F32))
    check(lib.rfi_op_roi_align_ml(ctx.handle, maps, case.N, case.H0, case.W0, case.C, D.ML_SCALE0, _P(dr), _P(dl), _P(dc), R, P_, P_, case.sr, _P(out)))
    ctx.synchronize()
    return out.numpy()


def _ml_backward(ctx, case, base, rois, lv, start, dout):
    dd = [ctx.to_device(np.ascontiguousarray(b, F32)) for b in base]
    dmaps = (C.c_void_p * 4)(*[a.ptr for a in dd])
    dr, dl, ds, ddo = ctx.to_device(rois), ctx.to_device(lv), ctx.to_device(start), ctx.to_device(dout)
    check(lib.rfi_op_roi_align_ml_backward(ctx.handle, dmaps, case.N, case.H0, case.W0, case.C, D.ML_SCALE0, _P(ddo), _P(dr), _P(dl), _P(ds),
                                           len(rois), case.P, case.P, case.sr))
    ctx.synchronize()
    return [a.numpy() for a in dd]


@pytest.mark.parametrize("case", D.ML_CASES, ids=lambda c: c.id)
def test_ml_roi_align_both_ways(case):
    ctx = _ctx()
    feats, rois, lv, start, dout = D.ml_inputs(case)
    R = len(rois)
    base = [np.random.default_rng(5 + k).standard_normal(f.shape).astype(F32) for k, f in enumerate(feats)]
    want, wantm = D.ml_reference(case, feats, rois, lv, dout, base, loops=True)
    r32, rm32 = D.ml_reference(case, feats, rois, lv, dout, base, F32)
    got = _ml_forward(ctx, case, feats, rois, lv, R)
    e_f = float(np.abs(r32 - want).max())
    bf = D.roi_bound(e_f, want)
    df = float(np.abs(got - want).max())
    assert got.tobytes() == _ml_forward(ctx, case, feats, rois, lv, R).tobytes()
    assert (_ml_forward(ctx, case, feats, rois, lv, 0) == 7.0).all()                 # count_dev = 0: nothing is written
    gotm = _ml_backward(ctx, case, base, rois, lv, start, dout)
    assert _same_bits(gotm, _ml_backward(ctx, case, base, rois, lv, start, dout))
    ratios, e_bs = [], []
    for k in range(4):
        e_b = float(np.abs(rm32[k] - wantm[k]).max())
        bb = D.roi_bound(e_b, wantm[k])
        ratios.append(float(np.abs(gotm[k] - wantm[k]).max()) / bb)
        e_bs.append(_u24(e_b, np.abs(wantm[k]).max()))
    # adjointness on zeroed maps: <forward(x), dout> = sum over the levels of <x_k, backward(dout)_k>, within the bounds of both
    zero = [np.zeros_like(b) for b in base]
    grads = _ml_backward(ctx, case, zero, rois, lv, start, dout)
    (_, wantg), (_, rg32) = D.ml_reference(case, feats, rois, lv, dout, zero, F64), D.ml_reference(case, feats, rois, lv, dout, zero, F32)
    lhs = float((got.astype(F64) * dout).sum())
    rhs = sum(float((g.astype(F64) * f).sum()) for g, f in zip(grads, feats))
    slack = bf * float(np.abs(dout).sum()) + sum(D.roi_bound(float(np.abs(r - w).max()), w) * float(np.abs(f).sum())
                                                 for r, w, f in zip(rg32, wantg, feats))
    print(f"DETEDGE {case.id} dfwd/bound={df / bf:.2f} dbwd/bound={max(ratios):.2f} e_ref={_u24(e_f, np.abs(want).max()):.2f}/{max(e_bs):.2f}u24 "
          f"adjoint={abs(lhs - rhs):.2e} (allowed {slack:.2e})")
    assert df <= bf, (df, bf)
    assert max(ratios) <= 1.0, ratios
    assert abs(lhs - rhs) <= slack, (lhs, rhs)


@pytest.mark.parametrize("Cc,PH,PW,word", [(1028, 7, 7, "1024"), (8, 33, 7, "32"), (8, 7, 33, "32")])
def test_ml_backward_refuses_what_its_lanes_cannot_hold(Cc, PH, PW, word):
    ctx = _ctx()
    dd = [ctx.to_device(np.full((1, 8 >> k, 8 >> k, Cc), 3.0, F32)) for k in range(4)]
    dmaps = (C.c_void_p * 4)(*[a.ptr for a in dd])
    dout, rois = ctx.to_device(np.ones((1, PH, PW, Cc), F32)), ctx.to_device(np.array([[0, 2, 2, 20, 20]], F32))
    lvl, start = ctx.to_device(np.zeros(1, np.int32)), ctx.to_device(np.array([0, 1], np.int32))
    with pytest.raises(RfiHipError) as err:
        check(lib.rfi_op_roi_align_ml_backward(ctx.handle, dmaps, 1, 8, 8, Cc, D.ML_SCALE0, _P(dout), _P(rois), _P(lvl), _P(start), 1, PH, PW, 2))
    assert word in str(err.value), str(err.value)        # the message names the limit
    ctx.synchronize()
    assert all((a.numpy() == 3.0).all() for a in dd)     # and nothing was launched


# ------------------------------------------------------------------------------------------------------------ E
def _mask_targets(masks, rois, P_):
    ctx = _ctx()
    G, H, W = masks.shape
    dm, dr = ctx.to_device(masks), ctx.to_device(rois)
    out = ctx.to_device(np.full((len(rois), P_, P_), 9, np.uint8))
    check(lib.rfi_op_mask_targets(ctx.handle, _P(dm), G, H, W, _P(dr), len(rois), P_, P_, 2, _P(out)))
    ctx.synchronize()
    return out.numpy()


def test_mask_targets_exact_averages():
    m, rois = D.mask_inputs(), D.mask_exact_rois()
    v = D.mask_averages(m, rois, 4)
    got = _mask_targets(m, rois, 4)
    assert np.array_equal(got, (v >= 0.5).astype(np.uint8)), np.argwhere(got != (v >= 0.5))[:8]
    print(f"DETEDGE mask_exact outputs={v.size} on_threshold={int((v == 0.5).sum())} mismatches=0")


def test_mask_targets_random_rois():
    m, rois = D.mask_inputs(), D.mask_random_rois()
    v = D.mask_averages(m, rois, 14)
    got = _mask_targets(m, rois, 14)
    left = np.abs(v - 0.5) <= 2.0 ** -20
    assert left.mean() <= 1e-3 and np.array_equal(got[~left], (v >= 0.5).astype(np.uint8)[~left])
    print(f"DETEDGE mask_random outputs={v.size} left_out={int(left.sum())} mismatches=0")

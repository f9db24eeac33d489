"""Per-emitter instance targets of a generated batch: one simulator event -- a broadband chunk, a narrowband channel, a
burst row, a linear or a quadratic sweep -- is one instance, with its own mask, tight box and family.

    batch = sim.generate_batch(8, out="nhwc")
    targets = event_instances(batch, min_side=2, max_instances=16)       # InstanceTargets in HBM, classes 1 .. 5
    losses = MaskRCNN(6, 8, ...).train_step(images, targets)

The simulator knows every emitter: each pixel of the truth mask is a function of (seed, sample index, event, position), so
``rfi_sim_event_table`` / ``rfi_sim_instances`` (csrc/rfi_sim.hip) recompute every event's own pixels on the device, with
the pixel kernel's device functions, from the batch's event table and ``batch.origin``.  Connected components of the mask
cannot do this: crossing lines merge into one grid.  Nothing goes through the host except the instance counts, which
size the mask buffer.

One event is one instance: a sweep that wraps in frequency keeps one tight box, which may then span the band; a pixel
flagged by several events is in each of their masks; ``gibbs_ringing`` never changes the mask, so never the instances.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .simulator import SimBatch, event_slots

EVENT_CLASSES = ("background", "broadband", "narrowband", "burst", "linear_sweep", "quadratic_sweep")
_CLASS_MODES = {"single": 0, "family": 1}


def _origin(batch):
    """-> (n, T, F, S) of a SimBatch made by generate_batch (no device call)."""
    if not isinstance(batch, SimBatch):
        raise ValueError(f"expected the SimBatch of RFISimulator.generate_batch, got {type(batch).__name__}")
    if batch.origin is None:
        raise ValueError("this SimBatch has no origin: it was not made by RFISimulator.generate_batch")
    o = batch.origin
    return int(batch.mask.shape[0]), o.T, o.F, event_slots(o.T, o.F) - 1


def _time_rows(batch, who):
    if batch.rows != "time":
        raise ValueError(f"{who} describes events in the simulator's (time, channel) orientation -- boxes are (channel, time, channel, "
                         f"time) and masks (T, F) -- but this batch was injected with rows={batch.rows!r}, whose planes are "
                         "(channel, time): inject with rows='time' for instance targets (family_masks works on both)")


def _sim_args(batch):
    o = batch.origin
    return (batch.mask.ctx.handle, o.seed, o.first_sample, int(batch.mask.shape[0]), C.byref(o.params), C.c_void_p(o.power.ptr),
            C.c_void_p(batch.events.ptr))


def _table(batch, n, S):
    from .._lib import check, lib
    ctx = batch.mask.ctx
    area, box = ctx.empty((n, S), np.int32), ctx.empty((n, S, 4), np.int32)
    check(lib.rfi_sim_event_table(*_sim_args(batch), C.c_void_p(area.ptr), C.c_void_p(box.ptr)))
    return area, box


def event_table(batch):
    """-> (area (n, S) int32, box (n, S, 4) int32) ``DeviceArray``s, S = event_slots(T, F) - 1: column l - 1 is event slot l
    of ``batch.events`` (slot 0 is the header).  area: the pixels the event alone flags; box: (xmin, ymin, xmax, ymax)
    inclusive over them, x the channel and y the time row, (0, 0, 0, 0) for an event that flags nothing (an unused third
    broadband slot among them).  A clean batch has no events: S columns of zeros."""
    n, T, F, S = _origin(batch)
    _time_rows(batch, "event_table")
    ctx = batch.mask.ctx
    if batch.events is None or n == 0:
        area, box = ctx.empty((n, S), np.int32), ctx.empty((n, S, 4), np.int32)
        if n:
            area.zero_(); box.zero_()
        return area, box
    return _table(batch, n, S)


def family_masks(batch):
    """Per-family segmentation targets straight from the generator -> ``DeviceArray`` (n, T, F) uint8 on the batch's GPU:
    bit ``c - 1`` is set where an event of ``EVENT_CLASSES[c]`` (c = 1 .. 5) flags the pixel.  These are class-bit labels
    for ``UNet(8, 5, ...).set_targets("class_bits")``; ``bits != 0`` is ``batch.mask``, a pixel several families flag
    carries all their bits, and ``gibbs_ringing`` changes nothing.  One kernel (``rfi_sim_family_bits``): no instance
    mask is formed.  A clean batch has no events and gives zeros (a fill), an empty one nothing at all.  A batch of
    ``inject(rows="channel")`` gives (n, F, T), the orientation of its mask: the same kernel, then a byte-plane transpose."""
    n, T, F, _ = _origin(batch)
    ctx = batch.mask.ctx
    if batch.events is None or n == 0:
        bits = ctx.empty((n, T, F) if batch.rows == "time" else (n, F, T), np.uint8)
        if n:
            bits.zero_()
        return bits
    bits = ctx.empty((n, T, F), np.uint8)
    from .._lib import check, lib
    check(lib.rfi_sim_family_bits(*_sim_args(batch), C.c_void_p(bits.ptr)))
    if batch.rows == "channel":                             # the kernel writes (T, F): turn the byte planes into the batch's (F, T)
        turned = ctx.empty((n, F, T), np.uint8)
        check(lib.rfi_sim_transpose_planes(ctx.handle, C.c_void_p(bits.ptr), n, T, F, C.c_void_p(turned.ptr)))
        ctx.synchronize()                                   # (`bits` goes with this frame)
        return turned
    return bits


def event_instances(batch, min_area=1, min_side=1, max_instances=64, classes="family", instance_masks=True):
    """Instance targets for the detector straight from the generator: every event of ``batch`` that flags at least
    ``min_area`` pixels and whose box has both sides >= ``min_side`` is one instance; at most ``max_instances`` (1 .. 256)
    per sample, the largest first, ties to the smaller slot -> ``InstanceTargets`` on the batch's GPU, laid out as
    ``instances_from_masks`` lays them out.  ``component`` is the event slot (an index into ``batch.events[i]``),
    ``n_components_host`` the number of event slots.  ``classes="family"``: labels 1 .. 5 = ``EVENT_CLASSES`` (a detector of
    6 classes); ``"single"``: every instance is class 1.  ``instance_masks=False`` leaves ``masks`` out -- a full set of
    masks is ``count`` planes of T F bytes per sample; ``min_side=2`` drops the one-pixel-wide lines.

    The targets follow the batch as generated: later changes of the simulator's attributes do not reach them."""
    from ..components import MAX_INSTANCES, InstanceTargets, _positive, _read_ints
    min_area, min_side = _positive("min_area", min_area), _positive("min_side", min_side)
    if isinstance(max_instances, (bool, np.bool_)) or not isinstance(max_instances, (int, np.integer)) or \
            not 1 <= max_instances <= MAX_INSTANCES:
        raise ValueError(f"max_instances must be an integer in 1 .. {MAX_INSTANCES}, got {max_instances!r}")
    if not isinstance(classes, str) or classes not in _CLASS_MODES:
        raise ValueError(f"classes must be 'family' or 'single', got {classes!r}")
    n, T, F, S = _origin(batch)
    _time_rows(batch, "event_instances")
    G = int(max_instances)
    num_classes = len(EVENT_CLASSES) if classes == "family" else 2
    if n == 0 or batch.events is None:                      # nothing to select from (a clean batch has no events): no device call
        z = np.zeros(n, np.int32)
        return InstanceTargets((T, F), np.zeros((n, G, 4), np.float32), np.zeros((n, G), np.int32), z, z, z, np.zeros((n, G), np.int32),
                               np.zeros((0, T, F), np.uint8) if instance_masks else None, z, z, np.full(n, S),
                               num_classes=num_classes)
    ctx = batch.mask.ctx
    boxes, labels, component = ctx.empty((n, G, 4), np.float32), ctx.empty((n, G), np.int32), ctx.empty((n, G), np.int32)
    count, surv, base = ctx.empty((n,), np.int32), ctx.empty((n,), np.int32), ctx.empty((n,), np.int32)
    from .._lib import check, lib
    from ..runtime import P
    area, box = _table(batch, n, S)
    n_comp = np.full(n, S, np.int32)
    n_components, comp_base = ctx.to_device(n_comp), ctx.to_device(np.arange(n, dtype=np.int32) * S)
    check(lib.rfi_op_instances_select(ctx.handle, P(n_components), P(comp_base), P(area), P(box), n, min_area, min_side, G,
                                      P(boxes), P(labels), P(count), P(surv), P(base), P(component)))
    count_host, surv_host = _read_ints(ctx, count, n), _read_ints(ctx, surv, n)
    inst = ctx.empty((int(count_host.sum(dtype=np.int64)), T, F), np.uint8) if instance_masks else None
    check(lib.rfi_sim_instances(*_sim_args(batch), P(component), P(count), P(base), G, _CLASS_MODES[classes], P(labels),
                                P(inst) if inst is not None and inst.nbytes else None))
    return InstanceTargets((T, F), boxes, labels, count, surv, base, component, inst, count_host, surv_host, n_comp,
                           num_classes=num_classes)

"""Connected components of binary masks on the GPU (csrc/components.hip; the arithmetic is pinned in include/rfi_hip.h,
"connected components"): what turns the package's binary masks -- simulator masks, dataset labels, flagger output,
thresholded predictions -- into separate objects.

    labels, k = label_components(mask)                       # scipy.ndimage.label, bit for bit
    table = component_table(mask)                            # per plane: area (K,), box (K, 4) = xmin, ymin, xmax, ymax
    clean = remove_small_components(flags, min_area=4)       # despeckling: the isolated specks a flagger leaves behind
    targets = instances_from_masks(masks)                    # the detector's ground truth, assembled in HBM
    losses = detector.train_step(images, targets)

Every function takes ``(..., H, W)`` masks -- a NumPy array, a torch tensor or a ``DeviceArray``; bool, uint8 or any numeric
dtype, non-zero == foreground -- treats every leading axis as a batch of independent planes and never modifies its input.
``connectivity`` is 4 (edge neighbours) or 8 (edge and corner neighbours).  A plane's components are numbered 1 .. K by the
smallest linear index ``y W + x`` each contains.  There is no CPU path.

What comes down to the host: the number of components per plane after labelling, where a table is sized by it, and the
number of instances per plane after the selection, which sizes the instance masks.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import DEVICE, HOST, MASK_CODES, check, lib
from .runtime import DeviceArray, P, check_out, context_for, describe, is_torch, operand, torch

MAX_PLANE = 1 << 30
MAX_PLANES = 65535
MAX_INSTANCES = 256


def limits():
    """(tile height, tile width, pixels of one root count): the sizes at which the kernels' paths change -- a plane of at
    most one tile needs no border merge, one of at most one root count no scan across counts (host only)."""
    v = [C.c_int32() for _ in range(3)]
    check(lib.rfi_components_limits(*(C.byref(x) for x in v)))
    return tuple(int(x.value) for x in v)


# ---------------------------------------------------------------------------------------------- argument plumbing
def _check_masks(name, masks, connectivity):
    """-> (shape, n, H, W) after the checks every function starts with (no device call)."""
    if connectivity not in (4, 8) or isinstance(connectivity, (bool, np.bool_)):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    shape, dt, _, owner = describe(masks)
    if len(shape) < 2:
        raise ValueError(f"{name} must have shape (..., H, W) with ndim >= 2, got shape {shape}")
    h, w = shape[-2:]
    if h < 1 or w < 1 or h * w > MAX_PLANE:
        raise ValueError(f"{name}: needs H, W >= 1 and H W <= 2^30, got {h} x {w}")
    n = int(np.prod(shape[:-2], dtype=np.int64))
    if n > MAX_PLANES:
        raise ValueError(f"{name}: at most {MAX_PLANES} planes in one call, got {n}")
    if owner is not None and dt not in (np.dtype(np.uint8), np.dtype(np.bool_), np.dtype(np.float32)):
        raise ValueError(f"a device array of {name} must be uint8, bool or float32, got {dt}")
    return shape, n, h, w


def _positive(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(min(v, (1 << 31) - 1))


def _read_ints(ctx, dev, count):
    """The first `count` int32 of a device array, through the library's small read-back (512 values at a time)."""
    out = np.empty(count, np.int32)
    for i in range(0, count, 512):
        k = min(512, count - i)
        check(lib.rfi_readback_begin(ctx.handle, C.c_void_p(dev.ptr + 4 * i), 4 * k))
        check(lib.rfi_readback_end(ctx.handle, C.c_void_p(out.ctypes.data + 4 * i), 4 * k))
    return out


def _scratch(ctx, nbytes):
    """The context's grow-only scratch of this module: the labels and the workspace of a call whose result is something
    else.  The next call on the context's stream reuses it, so a loop pays for no allocation of that size."""
    s = getattr(ctx, "_components_scratch", None)
    if s is None or s.nbytes < nbytes:
        ctx._components_scratch = s = None              # (released first; the release waits for the work in flight)
        ctx._components_scratch = s = ctx.empty((nbytes,), np.uint8)
    return s


class _Labelled:
    """Labels of a stack in HBM and what follows from them.  ``labels_ptr``: int32 (n, H, W), in an array of its own
    (``labels``, when the labels are the result) or in the context's scratch."""

    def __init__(self, masks, n, h, w, connectivity, device, own_labels=False):
        self.ctx, self.n, self.h, self.w = context_for(device, masks), n, h, w
        ctx = self.ctx
        m = operand(masks, ctx, (np.uint8, np.float32), "nonzero", to_device=True)      # (the kernel reads HBM only)
        ptr, code, self._input = m.ptr, MASK_CODES[m.dtype], m.keep
        ws_bytes, lab_bytes = int(lib.rfi_components_ws_bytes(n, h, w)), (4 * n * h * w + 255) & ~255
        self.n_components = ctx.empty((n,), np.int32)
        if own_labels:
            self.labels = ctx.empty((n, h, w), np.int32)
            self.labels_ptr, ws = self.labels.ptr, _scratch(ctx, ws_bytes).ptr
        else:
            self.labels_ptr = _scratch(ctx, lab_bytes + ws_bytes).ptr
            ws = self.labels_ptr + lab_bytes
        check(lib.rfi_op_label_components(ctx.handle, C.c_void_p(ptr), code, n, h, w, connectivity, C.c_void_p(ws),
                                          C.c_void_p(self.labels_ptr), C.c_void_p(self.n_components.ptr)))

    def table(self):
        """Reads K per plane back and fills area (total,) and box (total, 4); -> K on the host."""
        ctx = self.ctx
        self.k_host = _read_ints(ctx, self.n_components, self.n)
        base = np.concatenate([[0], np.cumsum(self.k_host, dtype=np.int64)])
        if base[-1] >= 1 << 31:
            raise ValueError(f"{int(base[-1])} components in all: at most 2^31 - 1 in one call")
        self.total = int(base[-1])
        self.base_host = base[:-1].astype(np.int32)
        self.comp_base = ctx.to_device(self.base_host)
        self.area, self.box = ctx.empty((max(self.total, 1),), np.int32), ctx.empty((max(self.total, 1), 4), np.int32)
        check(lib.rfi_op_component_table(ctx.handle, C.c_void_p(self.labels_ptr), self.n, self.h, self.w, C.c_void_p(self.comp_base.ptr),
                                         self.total, C.c_void_p(self.area.ptr), C.c_void_p(self.box.ptr)))
        return self.k_host


# ---------------------------------------------------------------------------------------------- the functions
def label_components(masks, connectivity=8, out="host", device=None):
    """-> (labels, n_components): int32 labels of ``masks``' shape, 0 for background and 1 .. K per plane, and K with the
    leading shape -- ``scipy.ndimage.label(mask != 0, generate_binary_structure(2, 1 if connectivity == 4 else 2))`` of every
    plane.  ``out="host"``: NumPy arrays; ``out="device"``: two ``DeviceArray``s, and nothing is read back."""
    shape, n, h, w = _check_masks("masks", masks, connectivity)
    check_out(out)
    if n == 0:
        ctx = context_for(device, masks) if out == "device" else None
        return (ctx.empty(shape, np.int32), ctx.empty(shape[:-2], np.int32)) if ctx else (np.zeros(shape, np.int32),
                                                                                          np.zeros(shape[:-2], np.int32))
    lab = _Labelled(masks, n, h, w, connectivity, device, own_labels=out == "device")
    if out == "device":
        lab.labels.shape, lab.n_components.shape = shape, shape[:-2]
        lab.labels._keep = lab._input           # (work in flight reads the input: it lives as long as the labels)
        return lab.labels, lab.n_components
    labels = np.empty(shape, np.int32)
    check(lib.rfi_memcpy(lab.ctx.handle, labels.ctypes.data_as(C.c_void_p), HOST, C.c_void_p(lab.labels_ptr), DEVICE, labels.nbytes))
    return labels, lab.n_components.numpy().reshape(shape[:-2])


def component_table(masks, connectivity=8, device=None):
    """-> per plane (leading axes flattened) ``{"area": int32 (K,), "box": int32 (K, 4)}`` in label order, box =
    ``(xmin, ymin, xmax, ymax)`` inclusive.  This is the host form: K per plane is read back to size the table, then the
    table comes down."""
    _, n, h, w = _check_masks("masks", masks, connectivity)
    if n == 0:
        return []
    lab = _Labelled(masks, n, h, w, connectivity, device)
    k = lab.table()
    area, box = lab.area.numpy()[:lab.total], lab.box.numpy()[:lab.total]
    return [{"area": area[b:b + c].copy(), "box": box[b:b + c].copy()} for b, c in zip(lab.base_host.tolist(), k.tolist())]


def remove_small_components(flags, min_area, connectivity=8, out="host", device=None):
    """Despeckling: ``flags`` without the components of fewer than ``min_area`` pixels.

    ``out="host"``: the shape, dtype and kind of the input (NumPy for NumPy, a torch tensor on the input's device for torch),
    values 0 / 1 (False / True).  ``out="device"``: a uint8 ``DeviceArray`` of 0 / 1.  K per plane is read back on the way
    (it sizes the area table); with a device-resident input nothing else crosses PCIe."""
    shape, n, h, w = _check_masks("flags", flags, connectivity)
    min_area = _positive("min_area", min_area)
    check_out(out)
    ctx = None
    if n:
        lab = _Labelled(flags, n, h, w, connectivity, device)
        ctx = lab.ctx
        lab.table()
        res = ctx.empty(shape, np.uint8)
        check(lib.rfi_op_components_keep(ctx.handle, C.c_void_p(lab.labels_ptr), n, h, w, C.c_void_p(lab.comp_base.ptr),
                                         C.c_void_p(lab.area.ptr), min_area, C.c_void_p(res.ptr)))
        res._keep = lab
    if out == "device":
        return res if n else context_for(device, flags).empty(shape, np.uint8)
    host = res.numpy() if n else np.zeros(shape, np.uint8)
    if is_torch(flags):
        return torch.from_numpy(host).to(device=flags.device, dtype=flags.dtype)
    dt = describe(flags)[1]
    return host.view(np.bool_) if dt == np.bool_ else host.astype(dt, copy=False)


class InstanceTargets:
    """Per-instance ground truth of ``n`` planes in HBM, in the layout ``MaskRCNN.train_step`` works on (G = ``max_instances``):
    ``boxes`` float32 (n, G, 4) = (xmin, ymin, xmax + 1, ymax + 1), ``labels`` int32 (n, G) (1 kept, 0 padding), ``count`` (n,),
    ``n_survivors`` (n,) (> count: the plane had more than G instances and the smallest were cut), ``base`` (n,) (exclusive prefix
    sum of count), ``component`` (n, G) (the label of ``label_components`` each slot came from), ``masks`` uint8
    (sum of count, H, W) or None -- all ``DeviceArray``s -- plus the host copies ``count_host``, ``n_survivors_host`` and
    ``n_components_host``.  Slots are in descending area, ties by ascending label.  ``num_classes``: the classes the labels
    need, background included (2 here; 6 for the emitter families of ``core.event_instances``)."""

    def __init__(self, shape, boxes, labels, count, n_survivors, base, component, masks, count_host, n_survivors_host,
                 n_components_host, num_classes=2):
        self.shape = tuple(shape)                      # (H, W) of a plane
        self.num_classes = int(num_classes)
        self.boxes, self.labels, self.count, self.n_survivors, self.base, self.component, self.masks = \
            boxes, labels, count, n_survivors, base, component, masks
        self.count_host, self.n_survivors_host, self.n_components_host = (np.asarray(a, np.int32) for a in
                                                                          (count_host, n_survivors_host, n_components_host))

    def __len__(self):
        return len(self.count_host)

    @property
    def max_count(self) -> int:
        return int(self.count_host.max()) if len(self.count_host) else 0

    @property
    def total(self) -> int:
        return int(self.count_host.sum(dtype=np.int64))

    def to_list(self):
        """-> ``[{"boxes": (k, 4) float32, "labels": (k,) int64, "masks": (k, H, W) uint8}, ...]``, the list form
        ``train_step`` takes (needs the instance masks)."""
        if self.masks is None:
            raise ValueError("these targets were made with instance_masks=False")
        num = lambda a: a.numpy() if isinstance(a, DeviceArray) else np.asarray(a)  # noqa: E731
        boxes, labels, masks = num(self.boxes), num(self.labels), num(self.masks)
        h, w = self.shape
        masks = masks.reshape(-1, h, w)
        out, b = [], 0
        for i, k in enumerate(self.count_host.tolist()):
            out.append({"boxes": boxes[i, :k].astype(np.float32), "labels": labels[i, :k].astype(np.int64),
                        "masks": masks[b:b + k].astype(np.uint8)})
            b += k
        return out


def instances_from_masks(masks, connectivity=8, min_area=1, min_side=1, max_instances=64, instance_masks=True, device=None):
    """Instance targets for the detector from binary masks: every connected component that survives ``min_area`` (pixels)
    and ``min_side`` (both sides of its bounding box, pixels) is one instance of class 1; at most ``max_instances`` (1 .. 256)
    per plane, the largest first (``InstanceTargets``).  ``instance_masks=False`` leaves ``masks`` out.

    On simulator masks expect one large instance plus specks: crossing narrow- and broadband lines merge into one
    component.  The function is for labelled data whose emitters are separate; for the batches of ``RFISimulator``,
    ``core.event_instances`` gives one instance per emitter."""
    shape, n, h, w = _check_masks("masks", masks, connectivity)
    min_area, min_side = _positive("min_area", min_area), _positive("min_side", min_side)
    if isinstance(max_instances, (bool, np.bool_)) or not isinstance(max_instances, (int, np.integer)) or \
            not 1 <= max_instances <= MAX_INSTANCES:
        raise ValueError(f"max_instances must be an integer in 1 .. {MAX_INSTANCES}, got {max_instances!r}")
    G = int(max_instances)
    if n == 0:
        z = np.zeros(0, np.int32)
        return InstanceTargets((h, w), np.zeros((0, G, 4), np.float32), np.zeros((0, G), np.int32), z, z, z, np.zeros((0, G), np.int32),
                               np.zeros((0, h, w), np.uint8) if instance_masks else None, z, z, z)
    lab = _Labelled(masks, n, h, w, connectivity, device)
    ctx = lab.ctx
    k_host = lab.table()
    boxes, labels, component = ctx.empty((n, G, 4), np.float32), ctx.empty((n, G), np.int32), ctx.empty((n, G), np.int32)
    count, surv, base = ctx.empty((n,), np.int32), ctx.empty((n,), np.int32), ctx.empty((n,), np.int32)
    check(lib.rfi_op_instances_select(ctx.handle, P(lab.n_components), P(lab.comp_base), P(lab.area), P(lab.box), n, min_area, min_side, G,
                                      P(boxes), P(labels), P(count), P(surv), P(base), P(component)))
    count_host, surv_host = _read_ints(ctx, count, n), _read_ints(ctx, surv, n)
    inst = None
    if instance_masks:
        total = int(count_host.sum(dtype=np.int64))
        inst = ctx.empty((total, h, w), np.uint8)
        if total:
            check(lib.rfi_op_instance_masks(ctx.handle, C.c_void_p(lab.labels_ptr), n, h, w, P(component), P(count), P(base), G, P(inst)))
        inst._keep = lab
    return InstanceTargets((h, w), boxes, labels, count, surv, base, component, inst, count_host, surv_host, k_host)

"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the per-emitter targets (rfi_sim_event_table / rfi_sim_instances of
rfi_toolbox_amd/csrc/rfi_sim.hip; rfi_toolbox_amd.core.event_instances) on top of tests/rfisim_ref.RefSimulator.

After ``RefSimulator.generate_rfi`` the simulator holds the sample's event table and its Philox position; every event's own
mask is recomputed from the recorded events with the restatement's draw helpers, the way generate_rfi sets the mask.  Area,
inclusive box, class and the selection (keys ~area << 32 | slot: descending area, ties ascending slot) follow from the
masks.  One event is one instance.
"""
import functools

import numpy as np

import rfisim_ref as R

FAMILY = {R.S_BROAD: 1, R.S_NARROW: 2, R.S_BURST: 3, R.S_LINEAR: 4, R.S_QUAD: 5}


def slot_category(slot, T, F):
    """event slot (1 .. S) -> (category, index within it), the order of RFI_SIM_SLOTS"""
    NN, NB = int(F * 0.05), int(T * 0.1)
    if slot < 4:
        return R.S_BROAD, slot - 1
    if slot < 4 + NN:
        return R.S_NARROW, slot - 4
    if slot < 4 + NN + NB:
        return R.S_BURST, slot - 4 - NN
    if slot < 9 + NN + NB:
        return R.S_LINEAR, slot - 4 - NN - NB
    return R.S_QUAD, slot - 9 - NN - NB


def sweep_points(sim, slot):
    """[(t, unwrapped channel)] of a sweep slot, in point order"""
    T, F = sim.time_bins, sim.freq_bins
    cat, _ = slot_category(slot, T, F)
    e = sim.events[slot]
    if cat == R.S_LINEAR:
        return [((int(e["i0"]) + i) % T, int(int(e["i1"]) + float(e["v0"]) * i)) for i in range(T // 2)]
    return [((int(e["i0"]) + t) % T, int(e["i1"]) + int(e["i2"]) * (t ** 2) // 100) for t in range(T // 4)]


def event_masks(sim):
    """(S, T, F) bool: row l - 1 = the pixels event slot l alone flags.  ``sim``: a RefSimulator right after generate_rfi."""
    T, F = sim.time_bins, sim.freq_bins
    S = len(sim.events) - 1
    floor = sim.detect_floor
    out = np.zeros((S, T, F), dtype=bool)
    t_col, t_lin, f_lin = np.arange(T)[:, None], np.arange(T), np.arange(F)
    for slot in range(1, S + 1):
        cat, k = slot_category(slot, T, F)
        e = sim.events[slot]
        params = (float(e["s0"]), float(e["sdot"]), float(e["r0"]), float(e["phi0"]))
        m = out[slot - 1]
        if cat == R.S_BROAD:
            if k >= int(sim.events[0]["i0"]):
                continue
            start, width = int(e["i0"]), int(e["i1"])
            n_row = np.arange(start, start + width)[None, :]
            r = sim._words(sim._pixels(t_col, n_row), k, R.S_BROAD_PX)
            field = (R.uniform(0.5, 2.0, r[0], r[1]) * sim._power(r[2])) * np.exp(1j * sim._phase_grid(t_col, n_row, params))
            m[:, start:start + width] = np.abs(field) > floor
        elif cat == R.S_NARROW:
            r = sim._words(t_lin, k, R.S_NARROW_PT)
            field = (R.uniform(0.5, 2.0, r[0], r[1]) * float(e["v0"])) * np.exp(1j * sim._phase_grid(t_lin, int(e["i0"]), params))
            m[np.abs(field) > floor, int(e["i0"])] = True
        elif cat == R.S_BURST:
            r = sim._words(f_lin, k, R.S_BURST_PT)
            field = (R.uniform(0.5, 2.0, r[0], r[1]) * float(e["v0"])) * np.exp(1j * sim._phase_grid(int(e["i0"]), f_lin, params))
            m[int(e["i0"]), np.abs(field) > floor] = True
        else:
            pts = sweep_points(sim, slot)
            amps = sim._power(sim._words(np.arange(len(pts)), k, R.S_LINEAR_PT if cat == R.S_LINEAR else R.S_QUAD_PT)[0])
            for (t, fu), amp in zip(pts, amps):
                if amp > floor:
                    m[t, fu % F] = True
    return out


def table(masks):
    """-> (area (S,) int32, box (S, 4) int32 = xmin, ymin, xmax, ymax inclusive; zeros for an empty event)"""
    S = len(masks)
    area, box = np.zeros(S, np.int32), np.zeros((S, 4), np.int32)
    for l, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        area[l] = len(ys)
        if len(ys):
            box[l] = (xs.min(), ys.min(), xs.max(), ys.max())
    return area, box


def classes(T, F, family=True):
    """class of every event slot 1 .. S"""
    S = 13 + int(F * 0.05) + int(T * 0.1)
    return np.array([FAMILY[slot_category(l, T, F)[0]] if family else 1 for l in range(1, S + 1)], np.int32)


def select(area, box, min_area=1, min_side=1, max_instances=64):
    """-> (slots kept, in output order; number of survivors): the header's rule, keys (~area << 32 | slot)"""
    w, h = box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1
    surv = np.nonzero((area >= min_area) & (w >= min_side) & (h >= min_side))[0] + 1
    keys = sorted(((0xFFFFFFFF - int(area[l - 1])) << 32 | int(l)) for l in surv)
    return [k & 0xFFFFFFFF for k in keys[:max_instances]], len(surv)


def targets(sample, min_area=1, min_side=1, max_instances=64, family=True):
    """One sample's expected InstanceTargets rows: dict of boxes (G, 4) float32, labels, component (G,) int32, count,
    n_survivors, masks (count, T, F) uint8."""
    G = max_instances
    kept, ns = select(sample["area"], sample["box"], min_area, min_side, G)
    T, F = sample["mask"].shape
    cls = classes(T, F, family)
    boxes, labels, comp = np.zeros((G, 4), np.float32), np.zeros(G, np.int32), np.zeros(G, np.int32)
    for j, l in enumerate(kept):
        b = sample["box"][l - 1]
        boxes[j] = (b[0], b[1], b[2] + 1, b[3] + 1)
        labels[j], comp[j] = cls[l - 1], l
    masks = sample["masks"][[l - 1 for l in kept]].astype(np.uint8) if kept else np.zeros((0, T, F), np.uint8)
    return {"boxes": boxes, "labels": labels, "component": comp, "count": len(kept), "n_survivors": ns, "masks": masks}


@functools.lru_cache(maxsize=None)
def case_reference(T, F, seed, n, detect_floor=1.0, first_sample=0):
    """The restatement's n samples of a case, computed once and shared (treat as read-only): per sample a dict of
    mask (T, F) bool, ambiguous, events, masks (S, T, F) bool, area, box."""
    sim = R.RefSimulator(T, F, seed=seed)
    sim.detect_floor = detect_floor
    sim.sample_counter = first_sample
    out = []
    for _ in range(n):
        sim.generate_rfi()
        masks = event_masks(sim)
        area, box = table(masks)
        out.append({"mask": sim.mask.copy(), "ambiguous": sim.ambiguous.copy(), "events": sim.events.copy(), "masks": masks,
                    "area": area, "box": box, "sweeps": {l: sweep_points(sim, l) for l in range(len(sim.events) - 10, len(sim.events))}})
    return out

"""TEST INFRASTRUCTURE ONLY -- the (T, F, seed, n_samples) cases of the per-emitter instance tests
(tests/test_sim_instances_host.py, tests/test_gpu_sim_instances.py) and why each is there."""

CASES = (
    (4, 52, 1, 3),        # the size floor: no burst rows, T/4 = 1 quadratic point, broadband width forced to 50
    (5, 53, 6, 2),        # T F = 265: instance planes start unaligned for 16-byte stores
    (7, 61, 7, 2),        # small odd shape
    (40, 64, 2, 3),       # small shape
    (128, 64, 3, 3),      # T > F: sweeps wrap many times, in both directions
    (96, 300, 4, 2),      # F crosses the pixel kernel's 256-column chunk and is no multiple of 16
    (128, 128, 5, 4),     # the detector's size
)
# beyond the table: T F = 34000 bytes, more than eight workgroups of the mask kernel (4 KiB each) and a cut last one
ODD_PLANE = (136, 250, 8, 1)
TALL = tuple(c for c in CASES if c[0] == 128)          # the 128-row cases: enough events for max_instances to cut


def case_id(case):
    return "T{}_F{}_seed{}_n{}".format(*case)

"""The cases of test_gpu_x3_accuracy.py: one per kernel VARIANT that implements the float32-by-3xbf16 arithmetic, at
shapes read off the dispatch code (launch_conv, launch_conv_ws, launch_gemm_ws, dispatch_tiles, launch_wgrad and the
select functions of wgrad_ws.hip), each with whole tiles and with ragged ones.  Plain data, importable without a GPU:
test_x3_probes_host.py builds every probe of every case on the CPU and checks that it tests something.

A case names the operation (x3_ref.OPS), the implementation code of the C ABI, the shape (n, h, w, cin, cout) as the ABI
takes it, the load transform (None / False: scale + shift / True: + ReLU) and the profile label the contraction launch
must carry: the kernel, its shape fields and the tile variant.  A shape that falls to another kernel fails on the label."""
from collections import namedtuple

IMPL_X3, IMPL_PX3, IMPL_WS = 4, 5, 7

Case = namedtuple("Case", "id row op impl shape relu label")
CASES = []


def _add(row, tag, op, impl, shape, label, relu=None):
    xf = {None: "", False: "-affine", True: "-bnrelu"}[relu]
    cid = f"{row}-{tag}-{op}-" + "x".join(str(v) for v in shape) + xf
    assert all(c.id != cid for c in CASES), cid
    CASES.append(Case(cid, row, op, impl, tuple(shape), relu, tuple(label)))


def _xf(relu):
    return "" if relu is None else " xf"


# ---------------------------------------------------------------- conv_ws (P = 3): conv3x3 / conv3x3_dgrad, IMPL_WS
# tile family by W (>= 32: 8x32, >= 16: 16x16, else four images of 8x8); ntl = 2 where Cout > 32 and
# tiles * ceil(ceil(Cout / 32) / 2) >= 224
def _conv_ws(tag, shape, tile, ntl, relu=None, dgrad=False):
    n, h, w, cin, cout = shape
    ci, co = (cout, cin) if dgrad else (cin, cout)          # the input gradient is a conv with the channels swapped
    _add("conv_ws", tag, "conv3x3_dgrad" if dgrad else "conv3x3", IMPL_WS, shape,
         [f"conv_ws N{n} {h}x{w} {ci}->{co}{_xf(relu)} 3xbf16", f" {tile} ntl{ntl}"], relu)


_conv_ws("8x32-whole", (2, 16, 32, 16, 32), "t8x32", 1)
_conv_ws("8x32-ragged", (1, 13, 37, 32, 48), "t8x32", 1, relu=True)
_conv_ws("16x16-whole", (2, 16, 16, 32, 64), "t16x16", 1, relu=True)
_conv_ws("16x16-ragged", (3, 19, 21, 16, 40), "t16x16", 1)
_conv_ws("4x8x8-whole", (4, 8, 8, 32, 32), "t4x8x8", 1)
_conv_ws("4x8x8-ragged", (5, 9, 11, 16, 72), "t4x8x8", 1, relu=False)
_conv_ws("8x32-ntl2", (4, 55, 127, 16, 128), "t8x32", 2, relu=True)           # 4*7*4 tiles * 2 column pairs = 224
_conv_ws("16x16-ntl2", (10, 40, 24, 16, 256), "t16x16", 2)                    # 10*3*2 * 4 = 240
_conv_ws("4x8x8-ntl2", (18, 20, 12, 16, 512), "t4x8x8", 2, relu=True)         # 5*3*2 * 8 = 240
_conv_ws("8x32-whole", (2, 16, 32, 32, 16), "t8x32", 1, dgrad=True)
_conv_ws("16x16-ragged", (3, 19, 21, 40, 16), "t16x16", 1, dgrad=True)
_conv_ws("4x8x8-ragged", (5, 9, 11, 72, 32), "t4x8x8", 1, dgrad=True)
_conv_ws("8x32-ntl2", (4, 55, 127, 128, 16), "t8x32", 2, dgrad=True)

# ---------------------------------------------------------------- conv_stem: conv3x3, IMPL_WS, Cin 4, Cout 32 / 64
for _tag, _shape in (("nt1-whole", (2, 16, 32, 4, 32)), ("nt1-ragged", (1, 13, 37, 4, 32)),
                     ("nt2-whole", (3, 8, 32, 4, 64)), ("nt2-ragged", (1, 21, 24, 4, 64))):
    _n, _h, _w, _, _co = _shape
    _add("conv_stem", _tag, "conv3x3", IMPL_WS, _shape, [f"conv_stem N{_n} {_h}x{_w} 4->{_co} 3xbf16"])


# ---------------------------------------------------------------- gemm_ws: convt2x2, convt2x2_dgrad, conv1x1, IMPL_WS
# 128-pixel tiles; column blocks of 32 GEMM channels (4 Cout for the transposed conv): 8 per workgroup ("wide") where
# there are more than 4 and tiles * ceil(blocks / 8) >= 192, else 2 (<= 2 blocks) or 4
def _gemm_ws(tag, op, shape, nb, relu=None):
    n, h, w, cin, cout = shape
    form, ci, co = {"convt2x2": ("convT", cin, cout), "convt2x2_dgrad": ("convT-dgrad", cout, cin),
                    "conv1x1": ("1x1", cin, cout)}[op]
    _add("gemm_ws", tag, op, IMPL_WS, shape, [f"gemm_ws {form} N{n} {h}x{w} {ci}->{co}{_xf(relu)} 3xbf16", f" {nb}"], relu)


_gemm_ws("nb4-whole", "convt2x2", (2, 8, 8, 16, 32), "nb4")
_gemm_ws("nb4-ragged", "convt2x2", (3, 5, 7, 48, 32), "nb4")
_gemm_ws("nb4-two-columns", "convt2x2", (2, 8, 8, 32, 64), "nb4")
_gemm_ws("wide", "convt2x2", (6, 64, 65, 16, 64), "nb8 wide")                 # 195 tiles, 8 blocks
_gemm_ws("nb2-whole", "convt2x2_dgrad", (2, 8, 8, 64, 32), "nb2")
_gemm_ws("nb2-ragged", "convt2x2_dgrad", (3, 5, 7, 40, 16), "nb2")
_gemm_ws("nb4", "convt2x2_dgrad", (1, 8, 8, 128, 32), "nb4")
_gemm_ws("wide", "convt2x2_dgrad", (6, 64, 65, 256, 16), "nb8 wide")
_gemm_ws("nb2-ragged", "conv1x1", (2, 7, 9, 48, 40), "nb2")
_gemm_ws("nb2-whole", "conv1x1", (1, 8, 32, 64, 64), "nb2", relu=True)
_gemm_ws("nb4-ragged", "conv1x1", (3, 5, 7, 32, 96), "nb4", relu=False)
_gemm_ws("wide", "conv1x1", (3, 64, 128, 16, 264), "nb8 wide", relu=True)      # 192 tiles, 9 blocks (the last one partial)


# ---------------------------------------------------------------- conv_igemm_kernel in the split arithmetic: IMPL_X3
# dispatch_tiles: W >= 32 / >= 16 / < 16 times Cout <= 32 / > 32 (the double tiles are not used in this arithmetic);
# the transposed conv with Cout % 4 == 0 runs folded (its four phases as 4 Cout channels), from 4 Cout >= 128 on the
# three 128-channel fold tiles
def _igemm(tag, op, shape, relu=None):
    n, h, w, cin, cout = shape
    r, ho, wo, ci, co, z4 = {
        "conv3x3": ("R3S1", h, w, cin, cout, ""), "conv3x3_dgrad": ("R3S1", h, w, cout, cin, ""),
        "conv1x1": ("R1S1", h, w, cin, cout, ""), "convt2x2": ("R1S1", h, w, cin, cout, " z4"),
        "convt2x2_dgrad": ("R2S2", h, w, cout, cin, ""),
        "conv_s2_k3": ("R2S1", h // 2, w // 2, 4 * cin, cout, ""), "conv_s2_k1": ("R1S1", h // 2, w // 2, cin, cout, ""),
        "conv_s2_k3_dgrad": ("R2S1", h // 2, w // 2, cout, 4 * cin, ""),
        "conv_s2_k1_dgrad": ("R1S1", h // 2, w // 2, cout, cin, "")}[op]
    _add("conv_igemm", tag, op, IMPL_X3, shape, [f"conv {r} N{n} {ho}x{wo} {ci}->{co}{_xf(relu)}{z4} 3xbf16"], relu)


_igemm("8x32x32-whole", "conv3x3", (2, 16, 32, 16, 32))
_igemm("4x32x64-ragged", "conv3x3", (1, 13, 37, 20, 48), relu=True)           # (Cin 20: a partial last 16-chunk)
_igemm("8x16x32-whole", "conv3x3", (2, 16, 16, 32, 32), relu=True)
_igemm("8x16x64-ragged", "conv3x3", (3, 19, 21, 12, 40))
_igemm("16x8x32-ragged", "conv3x3", (3, 9, 11, 20, 32), relu=False)
_igemm("8x8x64-whole", "conv3x3", (2, 8, 8, 32, 64))
_igemm("4x32x64-whole", "conv3x3_dgrad", (2, 16, 32, 64, 16))
_igemm("16x8x32-ragged", "conv3x3_dgrad", (3, 9, 11, 28, 20))
_igemm("fold-4x32x128", "convt2x2", (1, 8, 32, 16, 32))
_igemm("fold-8x16x128", "convt2x2", (2, 9, 17, 20, 36))
_igemm("fold-8x8x128", "convt2x2", (2, 5, 7, 16, 48))
_igemm("unfolded-tiles", "convt2x2", (2, 6, 10, 12, 20))                      # 4 Cout = 80 < 128: the general tiles
_igemm("whole", "convt2x2_dgrad", (1, 16, 32, 64, 32))
_igemm("ragged", "convt2x2_dgrad", (2, 6, 10, 12, 20))
for _op in ("conv_s2_k3", "conv_s2_k1", "conv_s2_k3_dgrad", "conv_s2_k1_dgrad"):
    _igemm("whole", _op, (2, 64, 64, 16, 48))
    _igemm("ragged", _op, (2, 12, 20, 20, 36))
_igemm("ragged", "conv1x1", (3, 5, 7, 36, 96))
_igemm("whole", "conv1x1", (1, 8, 32, 64, 32), relu=True)


# ---------------------------------------------------------------- the plane kernels with three planes: IMPL_PX3
def _planes(tag, op, shape, relu=None):
    n, h, w, cin, cout = shape
    k = lambda c: 16 * ((c + 15) // 16)
    label = {"conv3x3": [f"pconv N{n} {h}x{w} k{k(cin)}->{cout} 3xbf16"],
             "conv3x3_dgrad": [f"pconv N{n} {h}x{w} k{k(cout)}->{cin} 3xbf16"],
             "conv3x3_wgrad": [f"pwgrad R3 N{n} {h}x{w} cx{cin} cy{cout} split", " 3xbf16"]}[op]
    _add("planes", tag, op, IMPL_PX3, shape, label, relu)


for _op in ("conv3x3", "conv3x3_dgrad", "conv3x3_wgrad"):
    _planes("whole", _op, (2, 16, 32, 16, 32), relu=True if _op != "conv3x3_dgrad" else None)
    _planes("ragged-odd-channels", _op, (1, 13, 21, 6, 10))


# ---------------------------------------------------------------- wgrad_ws (P = 3): IMPL_X3 on the weight gradients
# label suffix: b<BYB>x<BXB> (32-channel blocks of dy / of x per workgroup), t<TH>x<TW> (pixel tile), xm<XM> (1: the
# compile-time BatchNorm + ReLU load transform, 2: run-time), pw8 (eight producer waves)
def _wgrad_ws(tag, op, shape, variant, relu=None):
    n, h, w, cin, cout = shape
    head = {"conv3x3_wgrad": f"wgrad_ws R3 N{n} {h}x{w} cx{cin} cy{cout} split",
            "conv_s2_k3_wgrad": f"wgrad_ws R2 N{n} {h // 2}x{w // 2} cx{4 * cin} cy{cout} split",
            "conv_s2_k1_wgrad": f"wgrad_ws R1 N{n} {h // 2}x{w // 2} cx{cin} cy{cout} split",
            "convt2x2_wgrad": f"wgrad_ws R2s2 N{n} {h}x{w} cx{cout} cy{cin} split"}[op]
    _add("wgrad_ws", tag, op, IMPL_X3, shape, [head, f" 3xbf16 {variant}"], relu)


# select<3>: (BYB, BXB) = (Cout > 32, Cin > 32); single blocks take an 8x16 tile for W >= 16, else 16x8
for _v, _whole, _ragged in (("b2x2 t8x8", (2, 16, 16, 64, 64), (3, 9, 11, 48, 72)),
                            ("b2x1 t8x8", (2, 16, 16, 32, 64), (1, 13, 19, 20, 40)),
                            ("b1x2 t8x8", (2, 8, 8, 64, 32), (3, 9, 11, 36, 20)),
                            ("b1x1 t8x16", (2, 16, 16, 32, 32), (1, 13, 19, 20, 12)),
                            ("b1x1 t16x8", (2, 16, 8, 16, 32), (3, 9, 11, 20, 12))):
    for _relu, _xm in ((None, 2), (True, 1)):
        _wgrad_ws("R3-whole", "conv3x3_wgrad", _whole, f"{_v} xm{_xm}", _relu)
        _wgrad_ws("R3-ragged", "conv3x3_wgrad", _ragged, f"{_v} xm{_xm}", _relu)
_wgrad_ws("R3-runtime-affine", "conv3x3_wgrad", (2, 16, 16, 32, 64), "b2x1 t8x8 xm2", False)
# select<2>: the 2x2 form of the strided 3x3 on its space-to-depth input (Cx = 4 Cin), pixels of the OUTPUT grid
_wgrad_ws("R2", "conv_s2_k3_wgrad", (2, 16, 16, 16, 64), "b2x2 t8x8 xm2")
_wgrad_ws("R2", "conv_s2_k3_wgrad", (2, 16, 16, 8, 64), "b2x1 t8x8 xm2")
_wgrad_ws("R2-ragged", "conv_s2_k3_wgrad", (3, 12, 20, 20, 12), "b1x2 t8x8 xm2")
_wgrad_ws("R2-ragged", "conv_s2_k3_wgrad", (1, 26, 40, 4, 16), "b1x1 t8x16 xm2")
_wgrad_ws("R2-ragged", "conv_s2_k3_wgrad", (2, 12, 20, 8, 32), "b1x1 t16x8 xm2")
# select<1>: the strided 1x1; 64 x 64 channels run the eight-producer form
_wgrad_ws("R1", "conv_s2_k1_wgrad", (2, 16, 16, 64, 64), "b2x2 t8x8 xm2 pw8")
_wgrad_ws("R1-ragged", "conv_s2_k1_wgrad", (3, 12, 20, 36, 40), "b2x2 t8x8 xm2 pw8")
_wgrad_ws("R1", "conv_s2_k1_wgrad", (2, 16, 16, 16, 64), "b2x1 t8x8 xm2")
_wgrad_ws("R1-ragged", "conv_s2_k1_wgrad", (2, 12, 20, 64, 16), "b1x2 t8x8 xm2")
_wgrad_ws("R1-ragged", "conv_s2_k1_wgrad", (1, 26, 40, 16, 16), "b1x1 t8x16 xm2")
_wgrad_ws("R1-ragged", "conv_s2_k1_wgrad", (2, 12, 20, 20, 12), "b1x1 t16x8 xm2")
# select_t2: the transposed conv (Yop = the layer input: BYB by Cin; Xop = dy: BXB by Cout), eight producer waves
for _v, _whole, _ragged in (("b2x2 t4x8", (2, 8, 8, 64, 64), (3, 5, 7, 48, 96)),
                            ("b2x1 t8x8", (2, 8, 8, 64, 32), (2, 9, 12, 36, 20)),
                            ("b1x2 t4x8", (2, 8, 8, 32, 64), (1, 7, 9, 16, 40)),
                            ("b1x1 t8x8", (2, 8, 8, 32, 32), (2, 5, 6, 16, 20))):
    _wgrad_ws("T2-whole", "convt2x2_wgrad", _whole, f"{_v} xm2 pw8")
    _wgrad_ws("T2-ragged", "convt2x2_wgrad", _ragged, f"{_v} xm2 pw8")

# ---------------------------------------------------------------- wgrad_stem: IMPL_X3 on conv3x3_wgrad, Cin 4
# launch_wgrad takes it where the slab workspace of the call holds 64 partial slabs, i.e. from 64 pixel tiles of
# wgrad_split's plan on (8x16 for Cout 32, 8x8 for Cout 64); a smaller stem-shaped call runs wgrad_ws (last two cases)
for _tag, _shape in (("cy32-whole", (2, 64, 64, 4, 32)), ("cy32-ragged", (3, 37, 70, 4, 32)),
                     ("cy64-whole", (1, 64, 64, 4, 64)), ("cy64-ragged", (2, 45, 52, 4, 64))):
    _n, _h, _w, _, _co = _shape
    _add("wgrad_stem", _tag, "conv3x3_wgrad", IMPL_X3, _shape, [f"wgrad_stem N{_n} {_h}x{_w} cx4 cy{_co} split", " 3xbf16"])
_wgrad_ws("R3-small-stem", "conv3x3_wgrad", (2, 16, 32, 4, 32), "b1x1 t8x16 xm2")
_wgrad_ws("R3-small-stem", "conv3x3_wgrad", (3, 8, 32, 4, 64), "b2x1 t8x8 xm2")

BY_ID = {c.id: c for c in CASES}
ROWS = ("conv_ws", "conv_stem", "gemm_ws", "conv_igemm", "planes", "wgrad_ws", "wgrad_stem")
assert {c.row for c in CASES} == set(ROWS)

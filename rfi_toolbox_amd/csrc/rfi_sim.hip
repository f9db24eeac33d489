// RFISimulator on device (rfi_toolbox/core/simulator.py:137-237): four-polarisation waterfalls with coherent
// per-event phase and full-truth masks down to a detectability floor, n samples per call, straight into HBM.
//
// Two launches.  rfisim_events_kernel draws every event's parameters (one thread per event slot) from
// Philox4x32-10 into a fixed-layout table (include/rfi_hip.h: rfi_sim_event and the word -> value mappings).
// rfisim_pixels_kernel then makes one gather per pixel: a workgroup owns a 256-column segment of one row, reads
// the sample's event table with scalar loads and adds, in fp64 and in the reference's order, noise + broadband +
// narrowband + bursts + linear sweeps (+ quadratic sweeps for RR), then RL/LR = noise + factor * RR.  A sweep
// is found per pixel in O(1): one sweep visits distinct rows, so the row gives the point index.  Every per-pixel
// and per-point value is keyed by (position, event, stream, global sample), so the result depends neither on
// the launch geometry nor on how the samples are split into calls.  No atomics: runs are bitwise reproducible.
//
// Gibbs ringing: a broadband pixel is a 17-tap convolution of its chunk's row.  Each field value costs a Philox
// block and an fp64 sincos, so recomputing it per tap would cost 17x; instead the workgroup stages the row
// segment of each chunk, with an 8-column halo on either side, in LDS (<= 3 chunks x 272 x 16 B) and every lane
// sums its 17 taps from there.  Narrowband / burst lines are one value per (event, row) or (event, column) and
// are evaluated by the lanes that need them.
//
// The gather itself is the device function gather_events, which rfisim_inject_kernel (rfi_sim_inject: the same events added
// to visibilities that already exist, at the data's noise scale) calls too, with another sink and, for (channel, time)
// planes, another tile.
//
// Per-emitter targets (below the pixel kernel): rfisim_event_table_kernel and rfisim_instance_masks_kernel recompute the
// pixels each event ALONE flags from the event table, through the device functions the pixel kernel decides its mask
// with -- one event is one instance of the detector's ground truth (include/rfi_hip.h, "per-emitter targets").
#include "kernels.hpp"
#include "philox.hpp"

namespace rfi {
namespace {

constexpr int kChunk = 256;          // columns per workgroup (= threads)
constexpr int kHalo = 8;             // Gibbs kernel half-width (n_side of _make_gibbs_kernel)
constexpr double kTwoPi = 6.283185307179586;     // 2 * np.pi

enum { S_HEADER = 0, S_BROAD = 1, S_NARROW = 2, S_BURST = 3, S_LINEAR = 4, S_QUAD = 5,
       S_NOISE = 8, S_BROAD_PX = 9, S_NARROW_PT = 10, S_BURST_PT = 11, S_LINEAR_PT = 12, S_QUAD_PT = 13,
       S_CROSS = 14 };


struct SimDev {
    unsigned k0, k1, first;          // key; global index of sample 0 (first + n <= 2^32)
    int n, T, F, NN, NB, slots, n_power, clean, fixed_bl, layout;
    double bl, floor, drift_prob, mtf, mff;
    double gk[17];
    const double* power;
    rfi_sim_event* ev;
    double* bl_out;
    void* out;
    uint8_t* mask;
};

__device__ __forceinline__ U4 draw(const SimDev& d, unsigned pos, unsigned event, unsigned stream, unsigned sample) {
    return philox4x32_10(U4{pos, event, stream, sample}, d.k0, d.k1);
}
// NumPy's random_sample from two words, and uniform(lo, hi) = lo + (hi - lo) * u
__device__ __forceinline__ double u53(unsigned a, unsigned b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}
__device__ __forceinline__ double uniform(double lo, double hi, unsigned a, unsigned b) { return lo + (hi - lo) * u53(a, b); }
__device__ __forceinline__ int randint(int lo, int hi, unsigned w) {
    return lo + (int)(((unsigned long long)w * (unsigned long long)(hi - lo)) >> 32);
}
__device__ __forceinline__ double sgn(unsigned w) { return (w >> 31) ? -1.0 : 1.0; }
__device__ __forceinline__ int power_index(unsigned w, int n) { return (int)(((unsigned long long)w * (unsigned)n) >> 32); }
__device__ __forceinline__ void normal2(unsigned a, unsigned b, double& n0, double& n1) {
    const double r = sqrt(-2.0 * log(((double)a + 1.0) * (1.0 / 4294967296.0)));
    double s, c;
    sincos(kTwoPi * ((double)b * (1.0 / 4294967296.0)), &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// _draw_event_phase (simulator.py:69-90) for an event of extent (width channels, ntimes rows)
__device__ void draw_phase(const SimDev& d, const unsigned* w, int width, int ntimes, bool drifting, double bl,
                           rfi_sim_event& e) {
    const double wd = (double)(width > 1 ? width : 1), nt = (double)(ntimes > 1 ? ntimes : 1);
    const double n_ft = uniform(0.5, 1.0 + bl * d.mtf, w[8], w[9]);
    e.r0 = (n_ft / nt) * sgn(w[10]);
    const double n_ff = uniform(0.5, 1.0 + bl * d.mff, w[12], w[13]);
    e.s0 = (n_ff / wd) * sgn(w[11]);
    e.phi0 = uniform(0.0, kTwoPi, w[14], w[15]);
    if (drifting) {
        const double s_end = (uniform(0.5, 1.0 + bl * d.mff, w[6], w[7]) / wd) * sgn(w[3]);
        e.sdot = (s_end - e.s0) / nt;
    } else {
        e.sdot = 0.0;
    }
}

// which event a table slot holds (the order of RFI_SIM_SLOTS): -> category S_HEADER .. S_QUAD, k = its index there
__device__ __forceinline__ int slot_category(int slot, int NN, int NB, int& k) {
    if (slot == 0) { k = 0; return S_HEADER; }
    if (slot < 4) { k = slot - 1; return S_BROAD; }
    if (slot < 4 + NN) { k = slot - 4; return S_NARROW; }
    if (slot < 4 + NN + NB) { k = slot - 4 - NN; return S_BURST; }
    if (slot < 9 + NN + NB) { k = slot - 4 - NN - NB; return S_LINEAR; }
    k = slot - 9 - NN - NB;
    return S_QUAD;
}

__global__ void rfisim_events_kernel(SimDev d) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)d.n * d.slots) return;
    const int s = (int)(gid / d.slots), slot = (int)(gid % d.slots);
    const unsigned sample = d.first + (unsigned)s;
    const int T = d.T, F = d.F;
    const U4 h = draw(d, 0, 0, S_HEADER, sample);
    const double bl = d.fixed_bl ? d.bl : u53(h.x, h.y);
    rfi_sim_event e{};
    int k;
    const int cat = slot_category(slot, d.NN, d.NB, k);
    unsigned w[20];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const U4 r = draw(d, (unsigned)j, (unsigned)k, (unsigned)cat, sample);
        w[4 * j] = r.x; w[4 * j + 1] = r.y; w[4 * j + 2] = r.z; w[4 * j + 3] = r.w;
    }
    switch (cat) {
    case S_HEADER:
        e.i0 = 2 + randint(0, 2, h.z);
        e.v0 = bl;
        if (d.bl_out) d.bl_out[s] = bl;
        break;
    case S_BROAD: {                  // simulator.py:163-168
        const int max_width = F - 1;
        e.i0 = randint(0, max(1, max_width - 100), w[0]);
        e.i1 = randint(50, min(150, max_width - e.i0), w[1]);
        e.i2 = u53(w[4], w[5]) < d.drift_prob;
        draw_phase(d, w, e.i1, T, e.i2 != 0, bl, e);
        break;
    }
    case S_NARROW:                   // :179-183
        e.i0 = randint(0, F, w[0]);
        e.i2 = power_index(w[1], d.n_power);
        e.v0 = d.power[e.i2];
        e.i1 = u53(w[4], w[5]) < d.drift_prob;
        draw_phase(d, w, 1, T, e.i1 != 0, bl, e);
        break;
    case S_BURST:                    // :193-196
        e.i0 = randint(0, T, w[0]);
        e.i2 = power_index(w[1], d.n_power);
        e.v0 = d.power[e.i2];
        draw_phase(d, w, F, 1, false, bl, e);
        break;
    case S_LINEAR:                   // :201-206
        e.i0 = randint(0, T / 2, w[0]);
        e.i1 = randint(0, F / 2, w[1]);
        e.v0 = uniform(-2.0, 2.0, w[16], w[17]);
        e.i2 = u53(w[4], w[5]) < d.drift_prob;
        draw_phase(d, w, 1, T / 2, e.i2 != 0, bl, e);
        break;
    default:                         // S_QUAD, :218-222
        e.i0 = randint(0, T / 4, w[0]);
        e.i1 = randint(0, F / 4, w[1]);
        e.i2 = (int)sgn(w[2]);
        draw_phase(d, w, 1, T / 4, true, bl, e);
        break;
    }
    d.ev[gid] = e;
}

// _phase_grid (:92-95) at (t, n)
__device__ __forceinline__ double phase(const rfi_sim_event& e, int t, int n) {
    return kTwoPi * ((e.s0 + e.sdot * (double)t) * (double)n + e.r0 * (double)t) + e.phi0;
}
// amp * exp(1j * phase): NumPy's complex product with a real amplitude is (amp cos, amp sin)
__device__ __forceinline__ double2 field(double amp, double ph) {
    double s, c;
    sincos(ph, &s, &c);
    return make_double2(amp * c, amp * s);
}
__device__ __forceinline__ double2 broadband_field(const SimDev& d, const rfi_sim_event& e, int b, int t, int f,
                                                   unsigned sample) {
    const U4 r = draw(d, (unsigned)t * (unsigned)d.F + (unsigned)f, (unsigned)b, S_BROAD_PX, sample);
    const double mod = uniform(0.5, 2.0, r.x, r.y);
    return field(mod * d.power[power_index(r.z, d.n_power)], phase(e, t, f));
}
// What one event deposits and where: the pixel kernel and the per-event kernels below (table, instance masks) decide
// "event e flags pixel (t, f)" through these and nothing else, so an event's own mask is the pixel kernel's term of it.
__device__ __forceinline__ double2 narrowband_field(const SimDev& d, const rfi_sim_event& e, int k, int t, unsigned sample) {
    const U4 r = draw(d, (unsigned)t, (unsigned)k, S_NARROW_PT, sample);
    return field(uniform(0.5, 2.0, r.x, r.y) * e.v0, phase(e, t, e.i0));
}
__device__ __forceinline__ double2 burst_field(const SimDev& d, const rfi_sim_event& e, int k, int f, unsigned sample) {
    const U4 r = draw(d, (unsigned)f, (unsigned)k, S_BURST_PT, sample);
    return field(uniform(0.5, 2.0, r.x, r.y) * e.v0, phase(e, e.i0, f));
}
__device__ __forceinline__ bool detectable(double2 v, double floor) { return hypot(v.x, v.y) > floor; }
// sweep point index of row t (a sweep visits distinct rows), < T/2 or T/4 on the sweep
__device__ __forceinline__ int sweep_point(const rfi_sim_event& e, int t, int T) { return (t - e.i0 + T) % T; }
// linear: channel int(start_f + slope i) % F
__device__ __forceinline__ int linear_channel(const rfi_sim_event& e, int i, int F) {
    const long long q = (long long)((double)e.i1 + e.v0 * (double)i);   // int(): toward zero
    int fi = (int)(q % F);
    if (fi < 0) fi += F;                                              // Python's % F
    return fi;
}
// quadratic: channel (start_f + (direction t^2) // 100) % F, floor division
__device__ __forceinline__ int quadratic_channel(const rfi_sim_event& e, int tt, int F) {
    const long long num = (long long)e.i2 * (long long)tt * (long long)tt;
    const long long fl = num >= 0 ? num / 100 : -((-num + 99) / 100);
    int fi = (int)(((long long)e.i1 + fl) % F);
    if (fi < 0) fi += F;
    return fi;
}
__device__ __forceinline__ double sweep_amp(const SimDev& d, int point, int k, unsigned stream, unsigned sample) {
    return d.power[power_index(draw(d, (unsigned)point, (unsigned)k, stream, sample).x, d.n_power)];
}
__device__ __forceinline__ void add(double2& acc, double2 v) {
    acc.x = acc.x + v.x;
    acc.y = acc.y + v.y;
}

// The event gather of one pixel (t, f) of sample s, shared by the generating kernel and the injecting one: every
// contribution in the reference's order -- broadband chunks, narrowband channels, burst rows, linear sweeps to
// sink.par (RR and LL), then the quadratic sweeps to sink.rr_only -- and the truth mask as the return value.  The
// workgroup's kChunk lanes tile TT rows x TF columns whose first pixel is (t0, f0); lane (lt, lf) of the tile owns
// (t, f) = (t0 + lt, f0 + lf) and `active` says that pixel exists.  Only the ringing broadband stage knows the tile:
// it stages each chunk's fields for the tile's rows with an 8-column halo in LDS.  Every lane of the workgroup must
// call this (a barrier and readlane broadcasts inside), and no draw depends on the tile shape.
template <bool RING, int TT, int TF, class Sink>
__device__ __forceinline__ bool gather_events(const SimDev& d, int s, unsigned sample, int t0, int f0, int lt, int lf, bool active,
                                              Sink& sink) {
    static_assert(TT * TF == kChunk, "a tile is one workgroup");
    constexpr int W = TF + 2 * kHalo;
    const int T = d.T, F = d.F, t = t0 + lt, f = f0 + lf;
    const rfi_sim_event* __restrict__ E = d.ev + (int64_t)s * d.slots;
    const int nbb = E[0].i0;
    const double floor = d.floor;
    bool m = false;
    // broadband chunks, in event order (:162-176)
    if (RING) {
        __shared__ double2 seg[3][TT][W];
        for (int b = 0; b < nbb; ++b) {
            const rfi_sim_event e = E[1 + b];
            const int lo = max(e.i0, f0 - kHalo), hi = min(e.i0 + e.i1, f0 + TF + kHalo);
            for (int idx = (int)threadIdx.x; idx < TT * W; idx += kChunk) {
                const int r = idx / W, w = idx - r * W, c = f0 - kHalo + w;
                if (c >= lo && c < hi && t0 + r < T) seg[b][r][w] = broadband_field(d, e, b, t0 + r, c, sample);
            }
        }
        __syncthreads();
        for (int b = 0; b < nbb; ++b) {
            const int c0 = E[1 + b].i0, c1 = c0 + E[1 + b].i1;
            if (active && f >= c0 && f < c1) {
                const double2 own = seg[b][lt][lf + kHalo];
                m = m || detectable(own, floor);
                // np.convolve(row, k, 'same'): out[f] = sum_c row[c] k[f - c + 8], zeros outside the chunk
                double2 acc = make_double2(0.0, 0.0);
                const int lo = max(c0, f - kHalo), hi = min(c1 - 1, f + kHalo);
                for (int c = lo; c <= hi; ++c) {
                    const double2 v = seg[b][lt][c - f0 + kHalo];
                    const double k = d.gk[f - c + kHalo];
                    acc.x = acc.x + v.x * k;
                    acc.y = acc.y + v.y * k;
                }
                sink.par(acc);
            }
        }
    } else {
        for (int b = 0; b < nbb; ++b) {
            const rfi_sim_event e = E[1 + b];
            if (active && f >= e.i0 && f < e.i0 + e.i1) {
                const double2 v = broadband_field(d, e, b, t, f, sample);
                m = m || detectable(v, floor);
                sink.par(v);
            }
        }
    }
    // narrowband channels (:178-188): the line value at row t, deposited on its channel or spread +-8 channels
    // (the channels / rows are fetched 64 at a time, one per lane, and broadcast with readlane: a dependent
    // scalar load per event would put one memory latency per event on every wave)
    const int lane = (int)(threadIdx.x & 63);
    for (int base = 0; base < d.NN; base += 64) {
        const int mine = base + lane < d.NN ? E[4 + base + lane].i0 : 0;
        const int cnt = min(64, d.NN - base);
        for (int j = 0; j < cnt; ++j) {
            const int k = base + j;
            const int df = f - __builtin_amdgcn_readlane(mine, j);
            if (active && (RING ? (df >= -kHalo && df <= kHalo) : df == 0)) {
                const rfi_sim_event e = E[4 + k];
                const double2 v = narrowband_field(d, e, k, t, sample);
                if (df == 0) m = m || detectable(v, floor);
                sink.par(RING ? make_double2(v.x * d.gk[df + kHalo], v.y * d.gk[df + kHalo]) : v);
            }
        }
    }
    // burst rows (:190-199)
    for (int base = 0; base < d.NB; base += 64) {
        const int mine = base + lane < d.NB ? E[4 + d.NN + base + lane].i0 : 0;
        const int cnt = min(64, d.NB - base);
        for (int j = 0; j < cnt; ++j) {
            const int k = base + j;
            const int dt = t - __builtin_amdgcn_readlane(mine, j);
            if (active && (RING ? (dt >= -kHalo && dt <= kHalo) : dt == 0)) {
                const rfi_sim_event e = E[4 + d.NN + k];
                const double2 v = burst_field(d, e, k, f, sample);
                if (dt == 0) m = m || detectable(v, floor);
                sink.par(RING ? make_double2(d.gk[dt + kHalo] * v.x, d.gk[dt + kHalo] * v.y) : v);
            }
        }
    }
    // linear sweeps (:201-214): point i = t - start_t, channel int(start_f + slope i) % F
    for (int k = 0; k < 5; ++k) {
        const rfi_sim_event e = E[4 + d.NN + d.NB + k];
        const int i = sweep_point(e, t, T);
        if (active && i < T / 2) {
            const int fi = linear_channel(e, i, F);
            if (f == fi) {
                const double amp = sweep_amp(d, i, k, S_LINEAR_PT, sample);
                sink.par(field(amp, phase(e, t, fi)));
                m = m || amp > floor;
            }
        }
    }
    // quadratic sweeps, RR only (:216-228): channel (start_f + (direction t^2) // 100) % F, floor division
    for (int k = 0; k < 5; ++k) {
        const rfi_sim_event e = E[9 + d.NN + d.NB + k];
        const int tt = sweep_point(e, t, T);
        if (active && tt < T / 4) {
            const int fi = quadratic_channel(e, tt, F);
            if (f == fi) {
                const double amp = sweep_amp(d, tt, k, S_QUAD_PT, sample);
                sink.rr_only(field(amp, phase(e, t, fi)));
                m = m || amp > floor;
            }
        }
    }
    return m;
}

// the generating kernel's sums: RR and LL start as their noise
struct GenSink {
    double2 rr, ll;
    __device__ __forceinline__ void par(double2 v) { add(rr, v); add(ll, v); }
    __device__ __forceinline__ void rr_only(double2 v) { add(rr, v); }
};

template <bool RING>
__global__ __launch_bounds__(kChunk) void rfisim_pixels_kernel(SimDev d) {
    const int nchunk = (d.F + kChunk - 1) / kChunk;
    const int64_t bid = blockIdx.x;
    const int chunk = (int)(bid % nchunk);
    const int64_t row = bid / nchunk;
    const int t = (int)(row % d.T), s = (int)(row / d.T);
    const int T = d.T, F = d.F, f0 = chunk * kChunk, f = f0 + (int)threadIdx.x;
    const bool active = f < F;
    const unsigned sample = d.first + (unsigned)s;
    const unsigned pix = (unsigned)t * (unsigned)F + (unsigned)(active ? f : 0);

    GenSink g;
    double2 rl, lr;
    {
        const U4 a = draw(d, pix, 0, S_NOISE, sample), b = draw(d, pix, 1, S_NOISE, sample);
        normal2(a.x, a.y, g.rr.x, g.rr.y);
        normal2(a.z, a.w, rl.x, rl.y);
        normal2(b.x, b.y, lr.x, lr.y);
        normal2(b.z, b.w, g.ll.x, g.ll.y);
    }
    bool m = false;
    if (!d.clean) {
        m = gather_events<RING, 1, kChunk>(d, s, sample, t, f0, 0, (int)threadIdx.x, active, g);
        // cross hands (:231-235)
        const U4 x = draw(d, pix, 0, S_CROSS, sample);
        const double frl = u53(x.x, x.y), flr = u53(x.z, x.w);
        rl.x = rl.x + frl * g.rr.x;
        rl.y = rl.y + frl * g.rr.y;
        lr.x = lr.x + flr * g.rr.x;
        lr.y = lr.y + flr * g.rr.y;
    }
    if (!active) return;
    const double2 rr = g.rr, ll = g.ll;
    const int64_t plane = (int64_t)T * F, px = (int64_t)t * F + f;
    d.mask[(int64_t)s * plane + px] = m ? 1 : 0;
    switch (d.layout) {
    case RFI_SIM_C128: {
        double2* o = reinterpret_cast<double2*>(d.out) + (int64_t)s * 4 * plane + px;
        o[0] = rr; o[plane] = rl; o[2 * plane] = lr; o[3 * plane] = ll;
        break;
    }
    case RFI_SIM_C64: {
        float2* o = reinterpret_cast<float2*>(d.out) + (int64_t)s * 4 * plane + px;
        o[0] = make_float2((float)rr.x, (float)rr.y);
        o[plane] = make_float2((float)rl.x, (float)rl.y);
        o[2 * plane] = make_float2((float)lr.x, (float)lr.y);
        o[3 * plane] = make_float2((float)ll.x, (float)ll.y);
        break;
    }
    case RFI_SIM_NCHW: {
        float* o = reinterpret_cast<float*>(d.out) + (int64_t)s * 8 * plane + px;
        o[0] = (float)rr.x; o[plane] = (float)rr.y; o[2 * plane] = (float)rl.x; o[3 * plane] = (float)rl.y;
        o[4 * plane] = (float)lr.x; o[5 * plane] = (float)lr.y; o[6 * plane] = (float)ll.x; o[7 * plane] = (float)ll.y;
        break;
    }
    default: {                       // RFI_SIM_NHWC: two 16-byte stores per pixel
        float4* o = reinterpret_cast<float4*>(d.out) + ((int64_t)s * plane + px) * 2;
        o[0] = make_float4((float)rr.x, (float)rr.y, (float)rl.x, (float)rl.y);
        o[1] = make_float4((float)lr.x, (float)lr.y, (float)ll.x, (float)ll.y);
        break;
    }
    }
}

// ---------------------------------------------------------------- injection into planes the simulator did not make
// rfi_sim_inject (include/rfi_hip.h): the same event table, the same gather and the same draws as above for (seed,
// first + s), added at the data's own noise scale sigma[s] to visibilities loaded from `data`; stream 8 (noise) is never
// drawn.  The planes are (T, F) (`CH` false: a workgroup is 256 channels of one row, as above) or (F, T) (`CH` true:
// simulator pixel (t, f) is element [f, t]).  There neighbouring lanes own neighbouring TIMES, so that a wave still reads
// and writes whole cache lines of every plane: 256 times of one channel without ringing, and with it a 16 x 16 tile whose
// 16 rows share one LDS stage of the +-8-channel broadband neighbourhood (each field value is then computed twice per tile,
// not 17 times; 16 complex128 are 256 contiguous bytes, 16 complex64 one 128-byte line).
struct InjDev {
    const void* data;                // (n, 4, R, S) complex128 / complex64; may be SimDev::out (in place)
    const uint8_t* flags;            // NULL, (n, 4, R, S) or (n, R, S): nonzero = stored as loaded
    const double* sigma;             // (n,)
    int flag_pols, cross, c64;
};

// the injecting kernel's sums: RR and LL start as loaded, S (RR's contributions alone) at zero; c = (sigma v.re, sigma v.im),
// each product rounded once and then added; t_rr / t_ll: something was added (x + 0 is not relied on to leave x alone)
struct InjectSink {
    double sigma;
    double2 rr, ll, S;
    bool t_rr, t_ll;
    __device__ __forceinline__ void par(double2 v) {
        const double2 c = make_double2(sigma * v.x, sigma * v.y);
        add(rr, c); add(ll, c); add(S, c);
        t_rr = true; t_ll = true;
    }
    __device__ __forceinline__ void rr_only(double2 v) {
        const double2 c = make_double2(sigma * v.x, sigma * v.y);
        add(rr, c); add(S, c);
        t_rr = true;
    }
};

__device__ __forceinline__ double2 widen(double2 z) { return z; }
__device__ __forceinline__ double2 widen(float2 z) { return make_double2((double)z.x, (double)z.y); }
__device__ __forceinline__ void narrow(double2 v, double2& z) { z = v; }
__device__ __forceinline__ void narrow(double2 v, float2& z) { z = make_float2((float)v.x, (float)v.y); }

// Z: the planes' element, double2 or float2.  Only RR and LL are loaded before the gather and only as loaded (their raw
// values are what an untouched or flagged visibility is stored from: bit for bit, NaN payloads included); RL, LR and the
// flags are loaded after it, so that the gather's loops run with few registers held across them.
template <bool RING, bool CH, class Z>
__global__ __launch_bounds__(kChunk) void rfisim_inject_kernel(SimDev d, InjDev q) {
    constexpr int TT = CH ? (RING ? 16 : kChunk) : 1, TF = kChunk / TT;
    const int T = d.T, F = d.F;
    const int nf = (F + TF - 1) / TF, nt = (T + TT - 1) / TT;
    const int64_t bid = blockIdx.x;
    const int cf = (int)(bid % nf);
    const int64_t rest = bid / nf;
    const int ct = (int)(rest % nt), s = (int)(rest / nt);
    const int tid = (int)threadIdx.x;
    const int lt = CH ? tid % TT : 0, lf = CH ? tid / TT : tid;          // the lane index runs along the planes' last axis
    const int t0 = ct * TT, f0 = cf * TF, t = t0 + lt, f = f0 + lf;
    const bool active = t < T && f < F;
    const unsigned sample = d.first + (unsigned)s;
    const unsigned pix = active ? (unsigned)t * (unsigned)F + (unsigned)f : 0u;
    const int64_t plane = (int64_t)T * F, px = active ? (CH ? (int64_t)f * T + t : (int64_t)t * F + f) : 0;
    const int64_t at = (int64_t)s * 4 * plane + px;
    const Z* in = reinterpret_cast<const Z*>(q.data);                    // (may be `out`: a thread reads a visibility, then writes it)
    Z* out = reinterpret_cast<Z*>(d.out);

    Z raw_rr{}, raw_ll{};
    if (active) {
        raw_rr = in[at];
        raw_ll = in[at + 3 * plane];
    }
    InjectSink g;
    g.sigma = q.sigma[s];
    g.rr = widen(raw_rr);
    g.ll = widen(raw_ll);
    g.S = make_double2(0.0, 0.0);
    g.t_rr = false;
    g.t_ll = false;
    const bool m = gather_events<RING, TT, TF>(d, s, sample, t0, f0, lt, lf, active, g);
    if (!active) return;
    const Z raw_rl = in[at + plane], raw_lr = in[at + 2 * plane];
    bool keep[4] = {false, false, false, false};
    if (q.flags) {
#pragma unroll
        for (int p = 0; p < 4; ++p) keep[p] = (q.flag_pols == 4 ? q.flags[at + p * plane] : q.flags[(int64_t)s * plane + px]) != 0;
    }
    // cross hands: the factors of the generating kernel's draw
    const U4 x = draw(d, pix, 0, S_CROSS, sample);
    const double frl = u53(x.x, x.y), flr = u53(x.z, x.w);
    double2 rl = widen(raw_rl), lr = widen(raw_lr);
    bool t_x;
    if (q.cross == RFI_INJECT_CROSS_REFERENCE) {                        // factor * the whole RR (:233-235)
        rl.x = rl.x + frl * g.rr.x;
        rl.y = rl.y + frl * g.rr.y;
        lr.x = lr.x + flr * g.rr.x;
        lr.y = lr.y + flr * g.rr.y;
        t_x = true;
    } else {                                                            // factor * what was injected into RR
        t_x = g.t_rr;
        if (t_x) {
            rl.x = rl.x + frl * g.S.x;
            rl.y = rl.y + frl * g.S.y;
            lr.x = lr.x + flr * g.S.x;
            lr.y = lr.y + flr * g.S.y;
        }
    }
    d.mask[(int64_t)s * plane + px] = m ? 1 : 0;
    Z z;
    narrow(g.rr, z);
    out[at] = keep[0] || !g.t_rr ? raw_rr : z;
    narrow(rl, z);
    out[at + plane] = keep[1] || !t_x ? raw_rl : z;
    narrow(lr, z);
    out[at + 2 * plane] = keep[2] || !t_x ? raw_lr : z;
    narrow(g.ll, z);
    out[at + 3 * plane] = keep[3] || !g.t_ll ? raw_ll : z;
}

// dst[i][c][r] = src[i][r][c] for n byte planes of R rows x C columns, through a 64 x 64 LDS tile so that both the reads
// and the writes of a wave are 64 consecutive bytes (family_masks of a rows="channel" batch)
constexpr int kTr = 64;
__global__ __launch_bounds__(256) void rfisim_transpose_bytes_kernel(const uint8_t* __restrict__ src, int R, int Cc, int tiles_r,
                                                                     int tiles_c, uint8_t* __restrict__ dst) {
    __shared__ uint8_t tile[kTr][kTr + 1];
    const int64_t bid = blockIdx.x;
    const int tc = (int)(bid % tiles_c);
    const int64_t rest = bid / tiles_c;
    const int tr = (int)(rest % tiles_r);
    const int64_t i = rest / tiles_r, plane = (int64_t)R * Cc;
    const int x = (int)(threadIdx.x & 63), y = (int)(threadIdx.x >> 6);
    const int r0 = tr * kTr, c0 = tc * kTr;
    for (int r = y; r < kTr; r += 4)
        if (r0 + r < R && c0 + x < Cc) tile[r][x] = src[i * plane + (int64_t)(r0 + r) * Cc + c0 + x];
    __syncthreads();
    for (int c = y; c < kTr; c += 4)
        if (c0 + c < Cc && r0 + x < R) dst[i * plane + (int64_t)(c0 + c) * R + r0 + x] = tile[x][c];
}

// ---------------------------------------------------------------- per-event targets: table, classes, instance masks
// One event is one instance.  Every pixel an event flags is recomputed from (seed, sample, event, position) with the
// device functions above, so nothing here reads the mask or the waterfalls, and nothing depends on the launch geometry.
constexpr int kTableBlock = 1024;    // threads of one (sample, slot) workgroup of the table kernel
constexpr int kRun = 16;             // bytes of an instance mask one thread owns: one 16-byte store

// pixels an event may flag: broadband width x T, narrowband T, burst F, linear T/2 points, quadratic T/4 points
__device__ __forceinline__ int64_t event_support(const SimDev& d, const rfi_sim_event& e, int cat) {
    switch (cat) {
    case S_BROAD: return (int64_t)e.i1 * d.T;
    case S_NARROW: return d.T;
    case S_BURST: return d.F;
    case S_LINEAR: return d.T / 2;
    case S_QUAD: return d.T / 4;
    default: return 0;
    }
}
// item `it` of the support -> its pixel (t, f) and whether the event flags it
__device__ __forceinline__ bool event_item(const SimDev& d, const rfi_sim_event& e, int cat, int k, int64_t it, unsigned sample,
                                           int& t, int& f) {
    switch (cat) {
    case S_BROAD:
        t = (int)(it / e.i1);
        f = e.i0 + (int)(it % e.i1);
        return detectable(broadband_field(d, e, k, t, f, sample), d.floor);
    case S_NARROW:
        t = (int)it;
        f = e.i0;
        return detectable(narrowband_field(d, e, k, t, sample), d.floor);
    case S_BURST:
        t = e.i0;
        f = (int)it;
        return detectable(burst_field(d, e, k, f, sample), d.floor);
    case S_LINEAR:
        t = (e.i0 + (int)it) % d.T;                    // sweep_point(e, t, T) == it
        f = linear_channel(e, (int)it, d.F);
        return sweep_amp(d, (int)it, k, S_LINEAR_PT, sample) > d.floor;
    default:                                           // S_QUAD
        t = (e.i0 + (int)it) % d.T;
        f = quadratic_channel(e, (int)it, d.F);
        return sweep_amp(d, (int)it, k, S_QUAD_PT, sample) > d.floor;
    }
}
// the event's flags on columns [fa, fb) of row t (fb - fa <= kRun): bit j = pixel (t, fa + j).  Only a broadband interior
// and the one column / row / point of a line event evaluate a draw.
__device__ __forceinline__ unsigned event_row_bits(const SimDev& d, const rfi_sim_event& e, int cat, int k, int t, int fa, int fb,
                                                   unsigned sample) {
    unsigned bits = 0;
    switch (cat) {
    case S_BROAD:
        for (int f = max(fa, e.i0), hi = min(fb, e.i0 + e.i1); f < hi; ++f)
            bits |= (unsigned)detectable(broadband_field(d, e, k, t, f, sample), d.floor) << (f - fa);
        break;
    case S_NARROW:
        if (e.i0 >= fa && e.i0 < fb) bits = (unsigned)detectable(narrowband_field(d, e, k, t, sample), d.floor) << (e.i0 - fa);
        break;
    case S_BURST:
        if (t == e.i0)
            for (int f = fa; f < fb; ++f) bits |= (unsigned)detectable(burst_field(d, e, k, f, sample), d.floor) << (f - fa);
        break;
    case S_LINEAR: {
        const int i = sweep_point(e, t, d.T);
        if (i < d.T / 2) {
            const int fi = linear_channel(e, i, d.F);
            if (fi >= fa && fi < fb) bits = (unsigned)(sweep_amp(d, i, k, S_LINEAR_PT, sample) > d.floor) << (fi - fa);
        }
        break;
    }
    case S_QUAD: {
        const int tt = sweep_point(e, t, d.T);
        if (tt < d.T / 4) {
            const int fi = quadratic_channel(e, tt, d.F);
            if (fi >= fa && fi < fb) bits = (unsigned)(sweep_amp(d, tt, k, S_QUAD_PT, sample) > d.floor) << (fi - fa);
        }
        break;
    }
    default: break;
    }
    return bits;
}
// the record of slot `slot` of sample s when it is a live event: a slot out of 1 .. slots - 1 and a broadband chunk the
// header does not use are no event
__device__ __forceinline__ bool live_event(const SimDev& d, int s, int slot, rfi_sim_event& e, int& cat, int& k) {
    if (slot < 1 || slot >= d.slots) return false;
    const rfi_sim_event* __restrict__ E = d.ev + (int64_t)s * d.slots;
    cat = slot_category(slot, d.NN, d.NB, k);
    if (cat == S_BROAD && k >= E[0].i0) return false;
    e = E[slot];
    return true;
}

// area and inclusive box of every event: one workgroup per (sample, slot 1 .. slots - 1); threads stride over the support,
// then a wave reduction and a fixed-order reduction of the waves' partial results in LDS
__global__ __launch_bounds__(kTableBlock) void rfisim_event_table_kernel(SimDev d, int* __restrict__ area, int* __restrict__ box) {
    __shared__ int part[kTableBlock / 64][5];
    const int S = d.slots - 1, s = (int)(blockIdx.x / S), slot = (int)(blockIdx.x % S) + 1;
    const unsigned sample = d.first + (unsigned)s;
    rfi_sim_event e;
    int cat = S_HEADER, k = 0;
    const bool live = live_event(d, s, slot, e, cat, k);
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    if (live) {
        const int64_t support = event_support(d, e, cat);
        for (int64_t it = threadIdx.x; it < support; it += kTableBlock) {
            int t, f;
            if (event_item(d, e, cat, k, it, sample, t, f)) {
                ++cnt;
                x0 = min(x0, f); x1 = max(x1, f);
                y0 = min(y0, t); y1 = max(y1, t);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_down(cnt, o);
        x0 = min(x0, __shfl_down(x0, o)); y0 = min(y0, __shfl_down(y0, o));
        x1 = max(x1, __shfl_down(x1, o)); y1 = max(y1, __shfl_down(y1, o));
    }
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = cnt; part[wave][1] = x0; part[wave][2] = y0; part[wave][3] = x1; part[wave][4] = y1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kTableBlock / 64; ++w) {
            cnt += part[w][0];
            x0 = min(x0, part[w][1]); y0 = min(y0, part[w][2]);
            x1 = max(x1, part[w][3]); y1 = max(y1, part[w][4]);
        }
        const int64_t o = (int64_t)s * S + slot - 1;
        area[o] = cnt;
        reinterpret_cast<int4*>(box)[o] = cnt ? make_int4(x0, y0, x1, y1) : make_int4(0, 0, 0, 0);
    }
}

// labels[i][j] = class of slot component[i][j], j < count[i]: 1, or the slot's category (1 broadband .. 5 quadratic)
__global__ void rfisim_instance_labels_kernel(SimDev d, const int* __restrict__ component, const int* __restrict__ count, int G,
                                              int family, int* __restrict__ labels) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)d.n * G) return;
    const int i = (int)(gid / G), j = (int)(gid % G);
    if (j >= count[i]) return;
    const int slot = component[gid];
    int k, cls = 0;
    if (slot >= 1 && slot < d.slots) cls = family ? slot_category(slot, d.NN, d.NB, k) : 1;
    labels[gid] = cls;
}

// masks[base[i] + j] = the pixels event component[i][j] alone flags, j < count[i], as a gather: a thread owns the kRun
// bytes of one 16-byte-aligned address range, works out the rows and columns they are, asks the event for its bits there
// and stores them once -- 16 bytes at a time inside a plane, byte by byte where the range is cut by the plane's first or
// last byte (planes are T F bytes apart, so all but the first may start unaligned; the neighbouring plane's thread
// writes the other bytes of that range).  One range per thread on purpose: a range inside a broadband chunk is 16 draws
// (Philox, fp64 sincos, hypot) one after the other, and a thread that walked eight ranges measured 2x slower.
// blockIdx: (instance slot i G + j) x blocks_per_plane + block of the plane.
__global__ __launch_bounds__(256) void rfisim_instance_masks_kernel(SimDev d, const int* __restrict__ component,
                                                                    const int* __restrict__ count, const int* __restrict__ base, int G,
                                                                    int blocks_per_plane, uint8_t* __restrict__ masks) {
    const int64_t inst = blockIdx.x / blocks_per_plane;
    const int i = (int)(inst / G), j = (int)(inst % G);
    if (j >= count[i]) return;
    const int64_t HW = (int64_t)d.T * d.F;
    uint8_t* plane = masks + ((int64_t)base[i] + j) * HW;
    const int head = (int)(reinterpret_cast<uintptr_t>(plane) & (kRun - 1));
    const int64_t c = (int64_t)(blockIdx.x % blocks_per_plane) * 256 + threadIdx.x;
    const int64_t r0 = c * kRun - head;                  // the range [r0, r0 + kRun) in the plane's pixel indices
    const int64_t p0 = max(r0, (int64_t)0), p1 = min(r0 + kRun, HW);
    if (p0 >= p1) return;
    rfi_sim_event e;
    int cat = S_HEADER, k = 0;
    unsigned bits = 0;                                   // bit b = pixel r0 + b
    if (live_event(d, i, component[(int64_t)i * G + j], e, cat, k)) {
        const unsigned sample = d.first + (unsigned)i;
        int t = (int)(p0 / d.F), f = (int)(p0 - (int64_t)t * d.F);
        for (int64_t p = p0; p < p1; ++t, f = 0) {
            const int fb = (int)min((int64_t)d.F, f + (p1 - p));
            bits |= event_row_bits(d, e, cat, k, t, f, fb, sample) << (int)(p - r0);
            p += fb - f;
        }
    }
    if (p1 - p0 == kRun) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned nib = (bits >> (4 * q)) & 15u;
            w[q] = (nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21;
        }
        *reinterpret_cast<uint4*>(plane + r0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int64_t p = p0; p < p1; ++p) plane[p] = (uint8_t)((bits >> (int)(p - r0)) & 1u);
    }
}

// bits[i] = one byte per pixel of sample i, bit cat - 1 set where an event of category cat (1 broadband .. 5 quadratic
// sweep) flags it: the OR by family of the instance masks, without the masks.  The same gather as above -- a thread owns one
// 16-byte-aligned range of the sample's plane and stores it once -- over every event slot of the sample: event_row_bits
// evaluates a draw only inside a broadband chunk and on the one column / row / point of a line event, so the slots that do
// not touch the range cost a few integer comparisons each.  blockIdx: sample x blocks_per_plane + block of the plane.
__global__ __launch_bounds__(256) void rfisim_family_bits_kernel(SimDev d, int blocks_per_plane, uint8_t* __restrict__ out) {
    const int i = (int)(blockIdx.x / blocks_per_plane);
    const int64_t HW = (int64_t)d.T * d.F;
    uint8_t* plane = out + (int64_t)i * HW;
    const int head = (int)(reinterpret_cast<uintptr_t>(plane) & (kRun - 1));
    const int64_t c = (int64_t)(blockIdx.x % blocks_per_plane) * 256 + threadIdx.x;
    const int64_t r0 = c * kRun - head;                  // the range [r0, r0 + kRun) in the plane's pixel indices
    const int64_t p0 = max(r0, (int64_t)0), p1 = min(r0 + kRun, HW);
    if (p0 >= p1) return;
    const unsigned sample = d.first + (unsigned)i;
    const int t0 = (int)(p0 / d.F), f0 = (int)(p0 - (int64_t)t0 * d.F);
    unsigned w[4] = {0, 0, 0, 0};                        // byte b of the range = byte b % 4 of w[b / 4]
    for (int slot = 1; slot < d.slots; ++slot) {
        rfi_sim_event e;
        int cat = S_HEADER, k = 0;
        if (!live_event(d, i, slot, e, cat, k)) continue;
        unsigned bits = 0;                               // bit b = pixel r0 + b
        int t = t0, f = f0;
        for (int64_t p = p0; p < p1; ++t, f = 0) {
            const int fb = (int)min((int64_t)d.F, f + (p1 - p));
            bits |= event_row_bits(d, e, cat, k, t, f, fb, sample) << (int)(p - r0);
            p += fb - f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned nib = (bits >> (4 * q)) & 15u;
            w[q] |= ((nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21) << (cat - 1);
        }
    }
    if (p1 - p0 == kRun) {
        *reinterpret_cast<uint4*>(plane + r0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int64_t p = p0; p < p1; ++p) {
            const int b = (int)(p - r0);
            plane[p] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
}

SimDev sim_dev(unsigned long long seed, unsigned first_sample, int n_samples, const rfi_sim_params& p, const double* power_dev,
               rfi_sim_event* events) {
    SimDev d{};
    d.k0 = (unsigned)seed;
    d.k1 = (unsigned)(seed >> 32);
    d.first = first_sample;
    d.n = n_samples;
    d.T = p.time_bins;
    d.F = p.freq_bins;
    d.NN = (int)((double)p.freq_bins * 0.05);
    d.NB = (int)((double)p.time_bins * 0.1);
    d.slots = RFI_SIM_SLOTS(p.time_bins, p.freq_bins);
    d.n_power = p.n_power;
    d.clean = p.clean ? 1 : 0;
    d.fixed_bl = p.fixed_baseline ? 1 : 0;
    d.bl = p.baseline_frac;
    d.floor = p.detect_floor;
    d.drift_prob = p.drift_prob;
    d.mtf = p.max_time_fringes;
    d.mff = p.max_freq_fringes;
    for (int i = 0; i < 17; ++i) d.gk[i] = p.gibbs_kernel[i];
    d.power = power_dev;
    d.ev = events;
    return d;
}

}  // namespace

void launch_rfi_sim(rfi_ctx* ctx, unsigned long long seed, unsigned first_sample, int n_samples,
                    const rfi_sim_params& p, const double* power_dev, int layout, void* out, uint8_t* mask,
                    rfi_sim_event* events, double* baseline_out) {
    SimDev d = sim_dev(seed, first_sample, n_samples, p, power_dev, events);
    d.layout = layout;
    d.bl_out = baseline_out;
    d.out = out;
    d.mask = mask;
    const int64_t px = (int64_t)n_samples * d.T * d.F;
    const int esz = layout == RFI_SIM_C128 ? 64 : 32;
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)px * (esz + 1));
    if (!d.clean) {
        const int64_t nt = (int64_t)n_samples * d.slots;
        hipLaunchKernelGGL(rfisim_events_kernel, dim3((unsigned)cdiv(nt, 256)), dim3(256), 0, ctx->stream, d);
        check_launch("rfisim_events");
    }
    const int64_t blocks = (int64_t)n_samples * d.T * cdiv(d.F, kChunk);
    if (p.gibbs_ringing && !d.clean)
        hipLaunchKernelGGL(rfisim_pixels_kernel<true>, dim3((unsigned)blocks), dim3(kChunk), 0, ctx->stream, d);
    else
        hipLaunchKernelGGL(rfisim_pixels_kernel<false>, dim3((unsigned)blocks), dim3(kChunk), 0, ctx->stream, d);
    check_launch("rfisim_pixels");
}

int64_t rfi_sim_inject_blocks(int n_samples, int T, int F, int ringing, int rows) {
    const int TT = rows == RFI_INJECT_ROWS_CHANNEL ? (ringing ? 16 : kChunk) : 1, TF = kChunk / TT;
    return (int64_t)n_samples * cdiv(T, TT) * cdiv(F, TF);
}

void launch_rfi_sim_inject(rfi_ctx* ctx, unsigned long long seed, unsigned first_sample, int n_samples, const rfi_sim_params& p,
                           const double* power_dev, int layout, int rows, int cross_hand, const void* data, const uint8_t* flags,
                           int flag_pols, const double* sigma, void* out, uint8_t* mask, rfi_sim_event* events, double* baseline_out) {
    SimDev d = sim_dev(seed, first_sample, n_samples, p, power_dev, events);
    d.clean = 0;
    d.layout = layout;
    d.bl_out = baseline_out;
    d.out = out;
    d.mask = mask;
    InjDev q{};
    q.data = data;
    q.flags = flags;
    q.sigma = sigma;
    q.flag_pols = flag_pols;
    q.cross = cross_hand;
    q.c64 = layout == RFI_SIM_C64 ? 1 : 0;
    const int64_t px = (int64_t)n_samples * d.T * d.F;
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)px * ((q.c64 ? 64 : 128) + 1 + (flags ? flag_pols : 0)));
    const int64_t nt = (int64_t)n_samples * d.slots;
    hipLaunchKernelGGL(rfisim_events_kernel, dim3((unsigned)cdiv(nt, 256)), dim3(256), 0, ctx->stream, d);
    check_launch("rfisim_events");
    const bool ring = p.gibbs_ringing != 0, ch = rows == RFI_INJECT_ROWS_CHANNEL;
    const dim3 grid((unsigned)rfi_sim_inject_blocks(n_samples, d.T, d.F, ring, rows)), block(kChunk);
    auto launch = [&](auto z) {
        using Z = decltype(z);
        if (ring && ch) hipLaunchKernelGGL((rfisim_inject_kernel<true, true, Z>), grid, block, 0, ctx->stream, d, q);
        else if (ring) hipLaunchKernelGGL((rfisim_inject_kernel<true, false, Z>), grid, block, 0, ctx->stream, d, q);
        else if (ch) hipLaunchKernelGGL((rfisim_inject_kernel<false, true, Z>), grid, block, 0, ctx->stream, d, q);
        else hipLaunchKernelGGL((rfisim_inject_kernel<false, false, Z>), grid, block, 0, ctx->stream, d, q);
    };
    if (q.c64) launch(float2{});
    else launch(double2{});
    check_launch("rfisim_inject");
}

void launch_rfi_sim_transpose_bytes(rfi_ctx* ctx, const uint8_t* src, int64_t n, int rows, int cols, uint8_t* dst) {
    const int64_t tr = cdiv(rows, kTr), tc = cdiv(cols, kTr);
    RFI_REQUIRE(n * tr * tc < ((int64_t)1 << 31), "sim_transpose_planes: batch too large for one launch");
    ProfScope ps(ctx, FAM_PREPROCESS, 0, 2.0 * (double)n * rows * cols);
    hipLaunchKernelGGL(rfisim_transpose_bytes_kernel, dim3((unsigned)(n * tr * tc)), dim3(256), 0, ctx->stream, src, rows, cols, (int)tr,
                       (int)tc, dst);
    check_launch("rfisim_transpose_bytes");
}

void launch_rfi_sim_event_table(rfi_ctx* ctx, unsigned long long seed, unsigned first_sample, int n_samples, const rfi_sim_params& p,
                                const double* power_dev, const rfi_sim_event* events, int* area, int* box) {
    RFI_REQUIRE(reinterpret_cast<uintptr_t>(box) % 16 == 0, "sim_event_table: box must be 16-byte aligned");
    const SimDev d = sim_dev(seed, first_sample, n_samples, p, power_dev, const_cast<rfi_sim_event*>(events));   // (read only here)
    const int64_t blocks = (int64_t)n_samples * (d.slots - 1);
    RFI_REQUIRE(blocks < ((int64_t)1 << 31), "sim_event_table: batch too large for one launch");
    ProfScope ps(ctx, FAM_PREPROCESS);
    hipLaunchKernelGGL(rfisim_event_table_kernel, dim3((unsigned)blocks), dim3(kTableBlock), 0, ctx->stream, d, area, box);
    check_launch("rfisim_event_table");
}

void launch_rfi_sim_instances(rfi_ctx* ctx, unsigned long long seed, unsigned first_sample, int n_samples, const rfi_sim_params& p,
                              const double* power_dev, const rfi_sim_event* events, const int* component, const int* count,
                              const int* base, int max_instances, int class_mode, int* labels, uint8_t* masks) {
    const SimDev d = sim_dev(seed, first_sample, n_samples, p, power_dev, const_cast<rfi_sim_event*>(events));   // (read only here)
    const int64_t slots = (int64_t)n_samples * max_instances, HW = (int64_t)d.T * d.F;
    const int64_t per_plane = cdiv(HW / kRun + 2, 256);          // ranges of a plane: at most HW / 16 whole ones and two cut ones
    RFI_REQUIRE(slots * per_plane < ((int64_t)1 << 31), "sim_instances: batch too large for one launch");
    ProfScope ps(ctx, FAM_PREPROCESS);
    hipLaunchKernelGGL(rfisim_instance_labels_kernel, dim3((unsigned)cdiv(slots, 256)), dim3(256), 0, ctx->stream, d, component, count,
                       max_instances, class_mode, labels);
    check_launch("rfisim_instance_labels");
    if (!masks) return;
    hipLaunchKernelGGL(rfisim_instance_masks_kernel, dim3((unsigned)(slots * per_plane)), dim3(256), 0, ctx->stream, d, component, count,
                       base, max_instances, (int)per_plane, masks);
    check_launch("rfisim_instance_masks");
}

void launch_rfi_sim_family_bits(rfi_ctx* ctx, unsigned long long seed, unsigned first_sample, int n_samples, const rfi_sim_params& p,
                                const double* power_dev, const rfi_sim_event* events, uint8_t* bits) {
    const SimDev d = sim_dev(seed, first_sample, n_samples, p, power_dev, const_cast<rfi_sim_event*>(events));   // (read only here)
    const int64_t HW = (int64_t)d.T * d.F;
    const int64_t per_plane = cdiv(HW / kRun + 2, 256);          // ranges of a plane: at most HW / 16 whole ones and two cut ones
    RFI_REQUIRE(n_samples * per_plane < ((int64_t)1 << 31), "sim_family_bits: batch too large for one launch");
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)n_samples * HW);
    hipLaunchKernelGGL(rfisim_family_bits_kernel, dim3((unsigned)(n_samples * per_plane)), dim3(256), 0, ctx->stream, d, (int)per_plane,
                       bits);
    check_launch("rfisim_family_bits");
}

}  // namespace rfi

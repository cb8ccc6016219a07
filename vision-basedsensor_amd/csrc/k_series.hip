// The time axis of the analysis layer: reductions ALONG TIME, PER MARKER, of the two dense tensors a tracked sequence ends as
// (table [N, M, 10], disp [n, M, 5]).  Float64 accumulation without contraction, no atomics: a result depends on its inputs
// only, never on the launch shape or on the order in which workgroups happen to run.
//   k_series_partial / k_series_finalize / k_series_cumsum   3d_reconstruction.py:332-334, 397-400 (analyze_displacement)
//   k_window_partial / k_window_finalize                     LocalAnalysis.py:53-60 (calculate_average_coordinates)
//   k_disp_from_frame                                        MarkerDisplacement.py:158-173 (SCALAR mode)
// The data is time-major: slot is the fast axis (stride 5 resp. 10 values), frame the slow one.  A thread owns ONE SLOT OF
// ONE CHUNK of VBS_SERIES_CHUNK frames, adjacent lanes read adjacent slots (a wave covers 64 consecutive rows of a frame),
// and the chunks of a slot are merged in frame order by one thread per slot (Chan, Golub & LeVeque's pairwise update).
// One wave per workgroup: 4096 frames x 169 slots are 128 x 3 workgroups, more than the part has compute units.
#include <cmath>

#include "common.h"
#pragma clang fp contract(off)

#define SER_CH VBS_SERIES_CHUNK
#define SER_REC VBS_SERIES_REC_COLS      // count, mean, M2, max, sum

// Chunks are aligned to GLOBAL frame 0: block x is global chunk frame_begin / SER_CH + x, cut to the call's frames
// [frame_begin, frame_begin + n) (so a call may begin or end inside a chunk: that record then covers a part of it).
// Within the chunk two passes (sum -> mean, then squared deviations; the second reads the rows from cache).
template <typename T>
__global__ __launch_bounds__(64) void k_series_partial(const T* __restrict__ disp, int n, int m_ref, int frame_begin,
                                                       double* __restrict__ rec) {
    const int slot = blockIdx.y * 64 + threadIdx.x;
    if (slot >= m_ref) return;
    const int64_t g0 = ((int64_t)(frame_begin / SER_CH) + blockIdx.x) * SER_CH;
    const int lo = (int)(g0 > frame_begin ? g0 - frame_begin : 0);
    const int hi = (int)(g0 + SER_CH < (int64_t)frame_begin + n ? g0 + SER_CH - frame_begin : n);
    const int64_t step = (int64_t)m_ref * VBS_DISP_COLS;
    const T* p0 = disp + (int64_t)lo * step + (int64_t)slot * VBS_DISP_COLS;
    double sum = 0.0, mx = -INFINITY;
    int cnt = 0;
    const T* p = p0;
    for (int f = lo; f < hi; ++f, p += step) {
        if (p[0] != (T)0) {
            const double x = (double)p[4];
            sum += x;
            mx = fmax(mx, x);
            ++cnt;
        }
    }
    const double mean = cnt ? sum / (double)cnt : 0.0;
    double m2 = 0.0;
    p = p0;
    for (int f = lo; f < hi; ++f, p += step) {
        if (p[0] != (T)0) {
            const double d = (double)p[4] - mean;
            m2 += d * d;
        }
    }
    double* r = rec + ((int64_t)blockIdx.x * m_ref + slot) * SER_REC;
    r[0] = (double)cnt; r[1] = mean; r[2] = m2; r[3] = mx; r[4] = sum;
}

// One thread per slot: the slot's records in the order given (= frame order), empty records skipped so that padding changes
// no bit.  stats row = count, mean, std (ddof = 1), max, total; count 0 -> the other four NaN, count 1 -> std NaN (what the
// reference's groupby gives: no group, resp. NaN).  The mean written is total / count, not the merged one: it then carries
// the plain bound of a sum of n terms; the merged mean only serves the update of M2.  prefix [n_rec][m_ref] (may be null) =
// the sum of the records before each one, which k_series_cumsum starts from.
__global__ __launch_bounds__(64) void k_series_finalize(const double* __restrict__ rec, int n_rec, int m_ref,
                                                        double* __restrict__ stats, double* __restrict__ prefix) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= m_ref) return;
    double na = 0.0, mean = 0.0, m2 = 0.0, mx = -INFINITY, tot = 0.0;
    for (int c = 0; c < n_rec; ++c) {
        const double* r = rec + ((int64_t)c * m_ref + slot) * SER_REC;
        if (prefix) prefix[(int64_t)c * m_ref + slot] = tot;
        const double nb = r[0];
        if (nb == 0.0) continue;
        if (na == 0.0) {
            mean = r[1]; m2 = r[2];
        } else {
            const double nn = na + nb, d = r[1] - mean;
            mean = mean + d * nb / nn;
            m2 = m2 + r[2] + d * d * na * nb / nn;
        }
        na += nb;
        mx = fmax(mx, r[3]);
        tot += r[4];
    }
    double* o = stats + (int64_t)slot * VBS_STATS_COLS;
    o[0] = na;
    o[1] = na > 0.0 ? tot / na : NAN;
    o[2] = na > 1.0 ? sqrt(m2 / (na - 1.0)) : NAN;
    o[3] = na > 0.0 ? mx : NAN;
    o[4] = na > 0.0 ? tot : NAN;
}

// The grid of k_series_partial: cumulative [n][m_ref] (float64) = the chunk's prefix + the running sum inside the chunk,
// inclusive; where the flag is 0 the running value is carried (those entries are no rows of the reference's DataFrame).
template <typename T>
__global__ __launch_bounds__(64) void k_series_cumsum(const T* __restrict__ disp, int n, int m_ref, int frame_begin,
                                                      const double* __restrict__ prefix, double* __restrict__ cum) {
    const int slot = blockIdx.y * 64 + threadIdx.x;
    if (slot >= m_ref) return;
    const int64_t g0 = ((int64_t)(frame_begin / SER_CH) + blockIdx.x) * SER_CH;
    const int lo = (int)(g0 > frame_begin ? g0 - frame_begin : 0);
    const int hi = (int)(g0 + SER_CH < (int64_t)frame_begin + n ? g0 + SER_CH - frame_begin : n);
    const int64_t step = (int64_t)m_ref * VBS_DISP_COLS;
    const T* p = disp + (int64_t)lo * step + (int64_t)slot * VBS_DISP_COLS;
    const double base = prefix[(int64_t)blockIdx.x * m_ref + slot];
    double run = 0.0;
    for (int f = lo; f < hi; ++f, p += step) {
        if (p[0] != (T)0) run += (double)p[4];
        cum[(int64_t)f * m_ref + slot] = base + run;
    }
}

// Window means: block (window, slot tile, piece of SER_CH frames counted from the window's first frame) -> part
// [window][piece][m_ref][4] = count, sum X, sum Y, sum Z over the rows with VBS_FLAG_XYZ; pieces past the window's end write 0.
struct WinArgs { int a[VBS_WINDOWS_PER_LAUNCH], b[VBS_WINDOWS_PER_LAUNCH]; };

__global__ __launch_bounds__(64) void k_window_partial(const float* __restrict__ table, int m_ref, WinArgs w, int pieces,
                                                       double* __restrict__ part) {
    const int slot = blockIdx.y * 64 + threadIdx.x;
    if (slot >= m_ref) return;
    const int win = blockIdx.x, piece = blockIdx.z;
    const int64_t lo = (int64_t)w.a[win] + (int64_t)piece * SER_CH;
    const int64_t hi = lo + SER_CH < (int64_t)w.b[win] + 1 ? lo + SER_CH : (int64_t)w.b[win] + 1;
    const int64_t step = (int64_t)m_ref * VBS_TABLE_COLS;
    const float* p = table + lo * step + (int64_t)slot * VBS_TABLE_COLS;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t f = lo; f < hi; ++f, p += step) {
        if ((int)p[0] & VBS_FLAG_XYZ) { s[0] += 1.0; s[1] += (double)p[6]; s[2] += (double)p[7]; s[3] += (double)p[8]; }
    }
    double* o = part + (((int64_t)win * pieces + piece) * m_ref + slot) * 4;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
}

// thread per (window, slot): the pieces summed in frame order -> means [window][m_ref][4] = count, mean X, Y, Z (NaN at count 0)
__global__ __launch_bounds__(64) void k_window_finalize(const double* __restrict__ part, int pieces, int m_ref,
                                                        double* __restrict__ means) {
    const int slot = blockIdx.y * 64 + threadIdx.x;
    if (slot >= m_ref) return;
    const int win = blockIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < pieces; ++q) {
        const double* r = part + (((int64_t)win * pieces + q) * m_ref + slot) * 4;
        s[0] += r[0]; s[1] += r[1]; s[2] += r[2]; s[3] += r[3];
    }
    double* o = means + ((int64_t)win * m_ref + slot) * VBS_WINDOW_COLS;
    o[0] = s[0];
    for (int c = 1; c < 4; ++c) o[c] = s[0] > 0.0 ? s[c] / s[0] : NAN;
}

// out [n][m_ref][2] = (flag, || P_f - P_ref ||) in float64; flag = both rows carry VBS_FLAG_XYZ (distance 0 where it is clear)
__global__ __launch_bounds__(256) void k_disp_from_frame(const float* __restrict__ table, int64_t rows, int m_ref, int ref_frame,
                                                         double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int slot = (int)(i % m_ref);
    const float* p = table + i * VBS_TABLE_COLS;
    const float* r = table + ((int64_t)ref_frame * m_ref + slot) * VBS_TABLE_COLS;
    const bool ok = ((int)p[0] & VBS_FLAG_XYZ) && ((int)r[0] & VBS_FLAG_XYZ);
    double d = 0.0;
    if (ok) {
        const double dx = (double)p[6] - (double)r[6], dy = (double)p[7] - (double)r[7], dz = (double)p[8] - (double)r[8];
        d = sqrt(dx * dx + dy * dy + dz * dz);
    }
    out[2 * i] = ok ? 1.0 : 0.0;
    out[2 * i + 1] = d;
}

// ---- launchers: h == nullptr (the float64 entry point has no handle) launches without the profiling brackets ----------------
#define SER_LAUNCH(h, s, name, ...)                                          \
    do {                                                                     \
        if (h) VBS_LAUNCH(h, s, name, __VA_ARGS__);                          \
        else hipLaunchKernelGGL(__VA_ARGS__);                                \
    } while (0)

static inline dim3 series_grid(int n, int m_ref, int frame_begin) {
    return dim3((unsigned)series_chunks(n, frame_begin), (unsigned)((m_ref + 63) / 64));
}

template <typename T>
static void series_partial_t(vbs_handle* h, const T* disp, int n, int m_ref, int frame_begin, double* rec, hipStream_t s) {
    SER_LAUNCH(h, s, "k_series_partial", k_series_partial<T>, series_grid(n, m_ref, frame_begin), dim3(64), 0, s, disp, n, m_ref,
               frame_begin, rec);
}

template <typename T>
static void series_cumsum_t(vbs_handle* h, const T* disp, int n, int m_ref, int frame_begin, const double* prefix, double* cum,
                            hipStream_t s) {
    SER_LAUNCH(h, s, "k_series_cumsum", k_series_cumsum<T>, series_grid(n, m_ref, frame_begin), dim3(64), 0, s, disp, n, m_ref,
               frame_begin, prefix, cum);
}

void launch_series_partial(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, double* rec, hipStream_t s) {
    series_partial_t(h, disp, n, m_ref, frame_begin, rec, s);
}
void launch_series_partial64(const double* disp, int n, int m_ref, int frame_begin, double* rec, hipStream_t s) {
    series_partial_t((vbs_handle*)nullptr, disp, n, m_ref, frame_begin, rec, s);
}
void launch_series_cumsum(vbs_handle* h, const float* disp, int n, int m_ref, int frame_begin, const double* prefix, double* cum,
                          hipStream_t s) {
    series_cumsum_t(h, disp, n, m_ref, frame_begin, prefix, cum, s);
}
void launch_series_cumsum64(const double* disp, int n, int m_ref, int frame_begin, const double* prefix, double* cum,
                            hipStream_t s) {
    series_cumsum_t((vbs_handle*)nullptr, disp, n, m_ref, frame_begin, prefix, cum, s);
}

void launch_series_finalize(vbs_handle* h, const double* rec, int n_rec, int m_ref, double* stats, double* prefix, hipStream_t s) {
    SER_LAUNCH(h, s, "k_series_finalize", k_series_finalize, dim3((unsigned)((m_ref + 63) / 64)), dim3(64), 0, s, rec, n_rec, m_ref,
               stats, prefix);
}

// nw <= VBS_WINDOWS_PER_LAUNCH windows [a, b] (inclusive, checked by the caller); part holds nw * pieces * m_ref * 4 doubles
void launch_window_means(vbs_handle* h, const float* table, int m_ref, const int32_t* windows, int nw, int pieces, double* part,
                         double* means, hipStream_t s) {
    WinArgs w{};
    for (int i = 0; i < nw; ++i) { w.a[i] = windows[2 * i]; w.b[i] = windows[2 * i + 1]; }
    const unsigned tiles = (unsigned)((m_ref + 63) / 64);
    VBS_LAUNCH(h, s, "k_window_partial", k_window_partial, dim3((unsigned)nw, tiles, (unsigned)pieces), dim3(64), 0, s, table, m_ref,
               w, pieces, part);
    VBS_LAUNCH(h, s, "k_window_finalize", k_window_finalize, dim3((unsigned)nw, tiles), dim3(64), 0, s, (const double*)part, pieces,
               m_ref, means);
}

void launch_disp_from_frame(vbs_handle* h, const float* table, int n, int m_ref, int ref_frame, double* out, hipStream_t s) {
    const int64_t rows = (int64_t)n * m_ref;
    VBS_LAUNCH(h, s, "k_disp_from_frame", k_disp_from_frame, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, table, rows,
               m_ref, ref_frame, out);
}

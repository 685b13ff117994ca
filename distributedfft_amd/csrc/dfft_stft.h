// dfft_stft.h -- host-side interface of the batched short-time Fourier transform and its inverse (dfft_stft.hip): rows of reals
// [rows][n] cut into frames of m reals that advance by `hop`, windowed and transformed (R2C), and the least-squares overlap-add back.
// Internal header (the C-ABI is include/dfft.h: dfft_stft1d, dfft_istft1d).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dfft {

enum StftPadMode { STFT_PAD_ZERO = 0, STFT_PAD_REFLECT = 1 };
enum StftOutKind { STFT_OUT_COMPLEX = 0, STFT_OUT_POWER = 1 };

// Frame f of row r is
//     xb[i] = P(in[r], f hop - pad + i) win[i]   (0 <= i < m;  P(row, s) = row[s] inside [0, n), else 0 (ZERO) or the mirrored sample
//                                                 row[-s] / row[2 (n - 1) - s] (REFLECT, which needs pad < n)),
//     out[r][f][k] = scale rfft(xb)[k] (COMPLEX: [rows][frames][m/2 + 1] complex)  or  scale^2 |rfft(xb)[k]|^2 (POWER: reals).
// 1 <= frames <= stft_frames(n, m, hop, pad).  in, out and win do not overlap; in and win are never written.
struct StftLaunch {
    int         dtype;  // DType: F64 = double, F32 = float
    int         pad_mode, out_kind;
    long long   n, m, hop, pad, frames, rows;
    double      scale;
    const void* in;
    void*       out;
    const void* win;
};

// out[r][t] = inv_env[t] sum_f win[t + pad - f hop] c_f[t + pad - f hop] / m over the f with 0 <= t + pad - f hop < m, where
// c_f = m irfft(in[r][f], m) (the imaginary parts of bins 0 and m/2 ignored); in [rows][frames][m/2 + 1] complex, out [rows][n] reals,
// 1 <= n <= (frames - 1) hop + m - pad.  in, win and inv_env are never written.
struct IstftLaunch {
    int         dtype;
    long long   n, m, hop, pad, frames, rows;
    const void* in;
    void*       out;
    const void* win;
    const void* inv_env;
};

// The two size rules that the entry points (dfft_stft_api.cpp) and the dispatcher (dfft_stft.hip) share, for rows, frames, hop >= 1:
// rows * frames items, fewer than 2^31
inline bool stft_items_ok(long long rows, long long frames) { return rows < (1ll << 31) && frames <= ((1ll << 31) - 1) / rows; }
// the inverse fills at most (frames - 1) hop + m - pad samples of a row; frames * hop is held below 2^62
inline bool istft_length_ok(long long n, long long m, long long hop, long long pad, long long frames) {
    return (__int128)frames * hop < ((__int128)1 << 62) && (__int128)n <= (__int128)(frames - 1) * hop + m - pad;
}
// 1 + (n + 2 pad - m) / hop where n + 2 pad >= m, else 0 (and 0 for sizes outside n >= 1, m >= 1, hop >= 1, 0 <= pad < m)
long long stft_frames(long long n, long long m, long long hop, long long pad);
// DFFT_STFT_FUSED (read per call): "0" forces the composed forward route
bool stft_fused_env();
// n, hop and pad even and `in` aligned to two reals: the fused kernel loads whole frames two reals at a time
bool stft_vec(const void* in, long long n, long long hop, long long pad, int dtype);
// One launch of stft_frames_kernel: m/2 has a tuned plan and stft_fused_ok keeps (m/2, dtype).  Depends on m and dtype only.
bool stft_fused(long long m, int dtype);
// Scratch bytes of one chunk of items (an item is one frame of one row) of at most max(cap, one item's), cap = 256 MiB (or
// DFFT_STFT_CHUNK_BYTES, the tests' way to make several chunks).  Forward: 0 for the fused kernel, else m reals per item (POWER: and
// its m/2 + 1 bins).  Inverse: m reals per item (untuned m/2: and a copy of its m/2 + 1 bins), and never fewer than the
// min(frames, ceil(m / hop)) items that one output sample sums.  0 for sizes that are refused.
size_t stft_scratch_bytes(const StftLaunch& L, bool fused_on);
size_t istft_scratch_bytes(const IstftLaunch& L);
// The transform of L: the fused kernel, or -- per chunk of items -- gather-and-window kernel, R2C rows (launch_real_rows) into `out`
// (POWER: into scratch bins, then the modulus kernel).  `scratch` holds scratch_bytes >= stft_scratch_bytes and aliases none of in,
// out, win.  Enqueues on `stream` only; allocates nothing (the twiddle tables are cached per device).  DFFT_OK or DFFT_E*.
int stft(const StftLaunch& L, bool fused_on, void* scratch, size_t scratch_bytes, hipStream_t stream);
// The inverse of L, per chunk of frames: C2R rows into scratch (after a copy of the bins where the two-launch C2R would merge in place
// on them), then the overlap-add gather kernel, one thread per output sample, frames summed in ascending order (no atomics).  Chunks
// hold whole rows where a row fits; a longer row is cut, and each cut transforms again the frames its first outputs share with the
// cut before.
int istft(const IstftLaunch& L, void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace dfft

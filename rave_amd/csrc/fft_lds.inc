// The frame-pair FFT stage of stft_loss.hip, mel.hip, spectrogram.hip, feed_mask.hip and inst_freq_loss.hip.  Included INSIDE the including file's
// anonymous namespace, after common.hpp; the device pieces come first, the host's checks and size dispatcher last.
//
//   * the transform: an in-LDS complex FFT, N = 128 ... 2048.  Stockham autosort, radix 8 (+ one radix 2 / 4 pass), N / 8 threads per
//     transform holding 8 points each, 256 / (N / 8) transforms per workgroup side by side; the LDS image is padded by one slot per
//     8 (zpad) so that the stride-8 stores of the first pass are conflict free; twiddles from a host-made table (f64 -> f32).
//     Written once for c32 (every unit's default) and c64 (Fft<N, c64> with an f64 table: inst_freq_loss.hip).
//   * the pair scheme: two real frames ride one transform as z = w (x + i y) and are split by X_k = (Z_k + conj Z_{n-k}) / 2,
//     Y_k = (Z_k - conj Z_{n-k}) / 2i (pair_split; each kernel walks the bin pairs itself).
//   * the equaliser (frame_scale, round 5): the two frames of a pair are EQUALISED first, y enters as s y with s = 2^(exponent of
//     max |x| over the frame - exponent of max |y|), exact in floating point, and Y = Y' / s after the transform.  A transform's
//     rounding error is ~ 1e-7 of the norm of its WHOLE input, so without this the quieter signal inherits the louder one's noise:
//     at the start of training the decoder's output is ~ 50x below the target and d log(|Y| + 1e-7) turned that noise into a
//     multiband gradient 60 % off the f64 value, where torch's separate f32 transforms are 0.3 % off
//     (profiles/round5_stft_pair_equalisation.txt); likewise the quiet frame of a pair at an onset (tests/test_gpu_mel.py).
//   * the packed scheme: a real frame u of 2 M = 4096 points is ONE M-point transform of z[m] = u[2m] + i u[2m + 1] (twiddles
//     from the 4096-point table: Tw::init<2>).  With Z its spectrum and W = e^{-2 pi i / 2M}: E_k = (Z_k + conj Z_{M-k}) / 2,
//     O_k = (Z_k - conj Z_{M-k}) / 2i (pair_split again: the even and the odd samples are the pair), U_k = E_k + W^k O_k,
//     U_{M-k} = conj(E_k - W^k O_k).

typedef float c32 __attribute__((ext_vector_type(2)));       // complex as a packed pair: adds / twiddle products are v_pk_* ops

// the same in double: the transform (cmul ... Fft below) is written once for both; inst_freq_loss.hip runs it on c64, every
// other unit on c32 (the default)
typedef double c64 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ c32 mk(float a, float b) { c32 r; r.x = a; r.y = b; return r; }
__device__ __forceinline__ c64 mk(double a, double b) { c64 r; r.x = a; r.y = b; return r; }
template <class C>
__device__ __forceinline__ C cmul(C a, C w) {
    C r = a.xx * w;
    return __builtin_elementwise_fma(a.yy, mk(-w.y, w.x), r);
}
template <class C>
__device__ __forceinline__ C mul_mi(C a) { return mk(a.y, -a.x); }          // a * (-i)

// forward DFTs (e^{-i}) of 2 / 4 / 8 points in natural order, in place on v[0], v[S], v[2S] ...
template <int S, class C>
__device__ __forceinline__ void dft2(C* v) {
    const C a = v[0], b = v[S];
    v[0] = a + b;
    v[S] = a - b;
}
template <int S, class C>
__device__ __forceinline__ void dft4(C* v) {
    const C b0 = v[0] + v[2 * S], b1 = v[0] - v[2 * S];
    const C b2 = v[S] + v[3 * S], b3 = mul_mi(C(v[S] - v[3 * S]));
    v[0] = b0 + b2;
    v[S] = b1 + b3;
    v[2 * S] = b0 - b2;
    v[3 * S] = b1 - b3;
}
template <class C>
__device__ __forceinline__ void dft8(C* v) {
    dft4<2>(v);          // even samples -> E_k at v[2k]
    dft4<2>(v + 1);      // odd samples  -> O_k at v[2k+1]
    constexpr decltype(C().x) kR = 0.70710678118654752440;
    const C e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    const C o0 = v[1];
    const C o1 = mk(v[3].x + v[3].y, v[3].y - v[3].x) * kR;         // * (1 - i) / sqrt 2
    const C o2 = mul_mi(v[5]);
    const C o3 = mk(v[7].y - v[7].x, -(v[7].x + v[7].y)) * kR;      // * (-1 - i) / sqrt 2
    v[0] = e0 + o0; v[4] = e0 - o0;
    v[1] = e1 + o1; v[5] = e1 - o1;
    v[2] = e2 + o2; v[6] = e2 - o2;
    v[3] = e3 + o3; v[7] = e3 - o3;
}
template <int R, class C>
__device__ __forceinline__ void dft(C* v) {
    if (R == 8) dft8(v);
    else if (R == 4) dft4<1>(v);
    else dft2<1>(v);
}

__device__ __forceinline__ int zpad(int i) { return i + (i >> 3); }

__device__ __forceinline__ int reflect_at(int p, int t) { return p < 0 ? -p : (p >= t ? 2 * (t - 1) - p : p); }

// the 8 samples n = t + r N/8 of frames f (-> .x) and f + 1 (-> .y) of one row, frame f starting at f hop - off; zero for a
// frame the workgroup does not own
template <int N>
__device__ __forceinline__ void load_pair(c32 (&v)[8], const float* __restrict__ xr, int t_len, int hop, int off, int f, bool va,
                                          bool vb, int t) {
    constexpr int TPF = N / 8;
    const int p0 = f * hop - off + t;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int q = p0 + r * TPF;
        const float a = va ? xr[reflect_at(q, t_len)] : 0.f;
        const float b = vb ? xr[reflect_at(q + hop, t_len)] : 0.f;
        v[r] = mk(a, b);
    }
}

// The pair split: X = hx (Z_k + conj Z_{n-k}), Y = hy (Z_k - conj Z_{n-k}) / i from z1 = Z_k, z2 = Z_{n-k}.  hx = 1/2 and
// hy = 1/2 x the equaliser's inverse give the two spectra; a caller's own scale goes INTO the prefactors (its rounding).
__device__ __forceinline__ void pair_split(c32 z1, c32 z2, float hx, float hy, c32& X, c32& Y) {
    X = mk(hx * (z1.x + z2.x), hx * (z1.y - z2.y));
    Y = mk(hy * (z1.y + z2.y), hy * (z2.x - z1.x));
}

// Equaliser of a frame pair: s = 2^(e_x - e_y) from the largest |x| and |y| of the frame (all N samples: the TPF threads of
// the transform; across waves through `fmx`, one slot per wave -- the barriers inside the transform that follows separate this
// read from the next frame's write), 1 when either frame is all zero.  Every thread of the workgroup must call it.
template <int TPF>
__device__ __forceinline__ void frame_scale(const c32 (&vn)[8], c32* fmx, float& s, float& inv_s, int on) {
    float mx = 0.f, my = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        mx = fmaxf(mx, fabsf(vn[r].x));
        my = fmaxf(my, fabsf(vn[r].y));
    }
    constexpr int W = TPF < 64 ? TPF : 64;
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        my = fmaxf(my, __shfl_xor(my, o, 64));
    }
    if (TPF > 64) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) fmx[wave] = mk(mx, my);
        __syncthreads();
        const int w0 = (threadIdx.x / TPF) * (TPF / 64);
        mx = my = 0.f;
#pragma unroll
        for (int i = 0; i < TPF / 64; ++i) {
            const c32 q = fmx[w0 + i];
            mx = fmaxf(mx, q.x);
            my = fmaxf(my, q.y);
        }
    }
    int d = (mx > 0.f && my > 0.f) ? (int)(__float_as_uint(mx) >> 23) - (int)(__float_as_uint(my) >> 23) : 0;
    d = d < -100 ? -100 : (d > 100 ? 100 : d);
    if (!on) d = 0;
    if (TPF >= 64) d = __builtin_amdgcn_readfirstlane(d);      // a whole wave works on one transform: the scale lives in an SGPR
    s = __uint_as_float((unsigned)(127 + d) << 23);
    inv_s = __uint_as_float((unsigned)(127 - d) << 23);
}

template <int N, class C = c32>
struct Fft {
    static constexpr int TPF = N / 8;                       // threads per transform
    static constexpr int G = 256 / TPF;                     // transforms per workgroup
    static constexpr int ZP = N + N / 8;                    // padded LDS image
    static constexpr int P8 = N >= 512 ? 3 : 2;             // radix-8 passes
    static constexpr int LAST = N / (P8 == 3 ? 512 : 64);   // then one pass of radix 2 / 4 (1: none)
    static constexpr int RF = LAST > 1 ? LAST : 8;          // radix of the final pass
    static constexpr int NSF = N / RF;
    static constexpr int NSL = LAST > 1 ? (P8 == 3 ? 512 : 64) : (P8 == 3 ? 64 : 8);    // NS of the final pass
    static constexpr bool MID2 = P8 == 3 && LAST > 1;       // a second middle pass (NS = 64)
    static constexpr int NTF = (RF - 1) * (8 / RF);

    // A transform's threads sit in ONE wave when TPF <= 64: LDS traffic of a wave is executed in order, no barrier needed
    static __device__ __forceinline__ void sync() {
        if (TPF > 64) __syncthreads();
        else __builtin_amdgcn_wave_barrier();
    }

    // every twiddle a thread ever needs depends on its index alone: fetched once, kept in registers across the frames
    struct Tw {
        C a[7];            // pass NS = 8
        C b[MID2 ? 7 : 1]; // pass NS = 64 (1024 / 2048 only)
        C f[NTF];          // final pass
        // `tw` holds e^{-2 pi i k / (S N)}, k < S N: S = 1 is the transform's own table, S = 2 the table of a real transform of
        // 2 N points packed into this one (feed_mask.hip), whose even entries are this transform's
        template <int S = 1>
        __device__ __forceinline__ void init(int t, const C* __restrict__ tw) {
#pragma unroll
            for (int r = 1; r < 8; ++r) a[r - 1] = tw[S * r * (t & 7) * (N / 64)];
            if (MID2) {
#pragma unroll
                for (int r = 1; r < 8; ++r) b[r - 1] = tw[S * r * (t & 63) * (N / 512)];
            }
#pragma unroll
            for (int u = 0; u < 8 / RF; ++u) {
                const int k = (t + u * TPF) & (NSL - 1);
#pragma unroll
                for (int r = 1; r < RF; ++r) f[u * (RF - 1) + r - 1] = tw[S * r * k * (N / (NSL * RF))];
            }
        }
    };

    // one Stockham pass: butterfly j = t + u TPF (u < 8 / R) takes in[j + r N/R], twiddles by e^{-2 pi i r k / (NS R)},
    // k = j mod NS, and its output r goes to (j - k) R + k + r NS.  With the padded index i + i/8 every address is a
    // per-thread base plus a compile-time constant (n/8 and NS >= 8 are multiples of 8): immediate offsets, no index math
    // per access.
    template <int R>
    static __device__ __forceinline__ void load(C (&v)[8], const C* z, int t, const C* w) {
        const C* zt = z + zpad(t);
#pragma unroll
        for (int u = 0; u < 8 / R; ++u) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                C a = zt[(u * TPF + r * (N / R)) / 8 * 9];
                if (r > 0) a = cmul(a, w[u * (R - 1) + r - 1]);
                v[u * R + r] = a;
            }
        }
    }
    template <int R>
    static __device__ __forceinline__ void bfly(C (&v)[8]) {
#pragma unroll
        for (int u = 0; u < 8 / R; ++u) dft<R>(&v[u * R]);
    }
    // radix-8 passes only (R = 8, one butterfly per thread: j = t)
    template <int NS>
    static __device__ __forceinline__ void store8(const C (&v)[8], C* z, int t) {
        const int k = t & (NS - 1);
        // NS = 1: 9 t + r;  NS = 8: 9 (t - k) + k + 9 r;  NS = 64: 9 (t - k) + k + k / 8 + 72 r
        C* zt = z + 9 * (t - k) + k + (k >> 3);
#pragma unroll
        for (int r = 0; r < 8; ++r) zt[NS == 1 ? r : r * NS / 8 * 9] = v[r];
    }
    template <int NS>
    static __device__ __forceinline__ void pass8(C (&v)[8], C* z, int t, const C* w) {
        load<8>(v, z, t, w);
        bfly<8>(v);
        sync();
        store8<NS>(v, z, t);
        sync();
    }
    // first pass with the 8 inputs v[r] = in[t + r TPF] already in registers; leaves everything but the final pass done
    // and returns with the final pass's butterflies in v: output r of butterfly u is sample (t + u TPF) + r NSF.
    // Every thread of the workgroup must call it (barriers); the caller guarantees nobody still reads z.
    static __device__ __forceinline__ void run(C (&v)[8], C* z, int t, const Tw& tw) {
        bfly<8>(v);
        store8<1>(v, z, t);
        sync();
        if (P8 == 3 || LAST > 1) pass8<8>(v, z, t, tw.a);
        if (MID2) pass8<64>(v, z, t, tw.b);
        load<RF>(v, z, t, tw.f);
        bfly<RF>(v);
        sync();                                             // all reads of z done: the caller may overwrite it
    }
    static __device__ __forceinline__ int out_index(int t, int u, int r) { return t + u * TPF + r * NSF; }
    // natural-order spectrum into z (barrier at the end)
    static __device__ __forceinline__ void store_natural(const C (&v)[8], C* z, int t) {
        C* zt = z + zpad(t);
#pragma unroll
        for (int u = 0; u < 8 / RF; ++u)
#pragma unroll
            for (int r = 0; r < RF; ++r) zt[(u * TPF + r * NSF) / 8 * 9] = v[u * RF + r];
        sync();
    }
};

// ---------------------------------------------------------------------------------------------------------------- host
// a built transform size up to `max_n` (2048, or 4096 where the unit has the packed scheme)
bool fft_size_ok(int n, int max_n) { return n >= 128 && n <= max_n && (n & (n - 1)) == 0; }

// fn(FftSize<n_fft>()) with the size as a compile-time constant; the caller has checked fft_size_ok(n_fft, MAX)
template <int N>
struct FftSize { static constexpr int value = N; };
template <int MAX, class Fn>
int fft_dispatch(int n_fft, Fn fn) {
    switch (n_fft) {
        case 128: return fn(FftSize<128>());
        case 256: return fn(FftSize<256>());
        case 512: return fn(FftSize<512>());
        case 1024: return fn(FftSize<1024>());
        case 2048: return fn(FftSize<2048>());
        default: return fn(FftSize<MAX>());      // 4096 where built; never another size: the caller's fft_size_ok
    }
}

// the twiddle table is read as c32; `what` (the operation's name) leads the message
int check_twiddle(const char* what, const void* twiddle) {
    RH_REQUIRE(twiddle && (reinterpret_cast<uintptr_t>(twiddle) & 7) == 0, RH_ERR_INVALID,
               "%s: the twiddle table must be non-null and 8-byte aligned", what);
    return RH_OK;
}
int check_scale(const char* what, float scale) {
    RH_REQUIRE(scale > 0.f && scale <= 3.4e38f, RH_ERR_INVALID, "%s: scale must be a positive finite number", what);
    return RH_OK;
}

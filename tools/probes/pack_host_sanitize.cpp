// The four HOST weight packers of include/dcvc_hip.h under AddressSanitizer + UBSan: a stand-alone program (its own main,
// nothing preloaded, no GPU touched -- the packers are pure host functions), linked with the host pass of the three
// convolution units.  Every buffer is a heap block of exactly the size the size function returns, so a write past the
// layout is an error report.  From the repository root, after `make -C vcm_ts_amd/csrc` (which leaves build/*.hipfb):
//
//   S="-Xarch_host -fsanitize=address,undefined"; C=vcm_ts_amd/csrc; F="--offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude"
//   for u in conv_mfma conv_k32 conv_small; do hipcc $F $S -cuid=dcvc_$u --offload-host-only -Xclang \
//       -fcuda-include-gpubinary -Xclang $C/build/$u.hipfb -c $C/$u.hip -o /tmp/$u.san.o; done
//   hipcc $F -fsanitize=address,undefined -x c++ tools/probes/pack_host_sanitize.cpp -x none /tmp/conv_*.san.o -o /tmp/pack_san
//   /tmp/pack_san
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dcvc_hip.h"

static std::vector<float> weights(int Cout, int Cin, int ks, bool special) {
    std::vector<float> w((size_t)Cout * Cin * ks * ks);
    uint32_t s = 12345u + Cout * 131 + Cin * 17 + ks;
    for (float &v : w) {
        s = s * 1664525u + 1013904223u;
        v = ((int)(s >> 8) % 2001 - 1000) * 1e-4f;
    }
    if (special) {  // range and non-finite values, a signed zero, a value whose lo part is an fp16 subnormal
        const float sp[6] = {1024.f, -1024.f, INFINITY, NAN, -0.f, 1e-6f};
        for (int i = 0; i < 6; ++i) w[i * ks * ks] = sp[i];
    }
    return w;
}

static unsigned sum(const void *p, int64_t bytes) {
    unsigned s = 0;
    for (int64_t i = 0; i < bytes; ++i) s = s * 31 + ((const unsigned char *)p)[i];
    return s;
}

int main() {
    int fails = 0;
    for (int special = 0; special < 2; ++special) {
        {  // plain layout: three segments with chunk tails, Cout 33 (pads to 64); then pixel shuffle with Cout 8
            const int32_t seg[3] = {17, 5, 32};
            for (int ps = 0; ps < 2; ++ps)
                for (int prec = 0; prec < 2; ++prec) {
                    const int Cout = ps ? 8 : 33;
                    int32_t cp = 0;
                    const int64_t n = dcvc_conv_pack_size(Cout, 3, 3, seg, &cp);
                    const std::vector<float> w = weights(Cout, 54, 3, special), b(Cout, 0.5f);
                    float *wp = (float *)malloc((size_t)n * 4), *bp = (float *)malloc((size_t)cp * 4);
                    const int rc = dcvc_conv_pack_weights(w.data(), b.data(), Cout, 3, 3, seg, ps, prec, wp, bp);
                    printf("plain ps %d prec %d special %d: rc %d sum %08x\n", ps, prec, special, rc, sum(wp, n * 4) ^ sum(bp, cp * 4));
                    fails += rc != DCVC_OK;  // the plain packer clamps silently
                    free(wp), free(bp);
                }
        }
        {  // tap-paired: Cin 3 (five empty channel slots per half), Cout 17
            int32_t cp = 0;
            const int64_t n = dcvc_conv_pack_size_paired(17, 3, &cp);
            const std::vector<float> w = weights(17, 3, 7, false);
            std::vector<float> w8 = weights(17, 8, 7, special);
            float *wp = (float *)malloc((size_t)n * 4), *bp = (float *)malloc((size_t)cp * 4);
            int rc = dcvc_conv_pack_weights_paired(w.data(), nullptr, 17, 3, wp, bp);
            fails += rc != DCVC_OK;
            rc = dcvc_conv_pack_weights_paired(w8.data(), nullptr, 17, 8, wp, bp);
            printf("paired special %d: rc %d sum %08x\n", special, rc, sum(wp, n * 4) ^ sum(bp, cp * 4));
            fails += rc != (special ? DCVC_E_RANGE : DCVC_OK);
            free(wp), free(bp);
        }
        {  // small: Cout 2, 7x7, segments (20, 16)
            const int32_t seg[2] = {20, 16};
            const int64_t n = dcvc_conv_small_pack_bytes(2, 7, 2, seg);
            const std::vector<float> w = weights(2, 36, 7, special);
            void *wp = malloc((size_t)n);
            float *bp = (float *)malloc(16 * 4);
            const int rc = dcvc_conv_small_pack_weights(w.data(), nullptr, 2, 7, 2, seg, wp, bp);
            printf("small special %d: rc %d sum %08x\n", special, rc, sum(wp, n) ^ sum(bp, 64));
            fails += rc != (special ? DCVC_E_RANGE : DCVC_OK);
            free(wp), free(bp);
        }
        {  // k32: Cout 12 with pixel shuffle, 3x3, segments (64, 32)
            const int32_t seg[2] = {64, 32};
            int32_t cp = 0;
            const int64_t n = dcvc_conv_k32_pack_bytes(12, 3, 2, seg, &cp);
            const std::vector<float> w = weights(12, 96, 3, special), b(12, -0.25f);
            void *wp = malloc((size_t)n);
            float *bp = (float *)malloc((size_t)cp * 4);
            const int rc = dcvc_conv_k32_pack_weights(w.data(), b.data(), 12, 3, 2, seg, 1, wp, bp);
            printf("k32 special %d: rc %d sum %08x\n", special, rc, sum(wp, n) ^ sum(bp, cp * 4));
            fails += rc != (special ? DCVC_E_RANGE : DCVC_OK);
            free(wp), free(bp);
        }
    }
    printf(fails ? "FAILED: %d unexpected status codes\n" : "ok\n", fails);
    return fails != 0;
}

// A stand-alone host check of the weight manifest (csrc/manifest.h) and the vocoders' weight packers (voc_pack_f32 of
// csrc/vocoder_common.h, gt_hifigan_pack16 of csrc/hifigan.hip), meant to be built with the host sanitizers; it never touches a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -x hip tools/manifest_check.cpp \
//         gst_tacotron_amd/csrc/hifigan.hip -o /tmp/manifest_check && /tmp/manifest_check
// Prints "manifest_check: ok" and returns 0, or says what differed and returns 1.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../gst_tacotron_amd/csrc/manifest.h"
#include "../gst_tacotron_amd/csrc/vocoder_common.h"

static std::string g_last;
int gt_fail(const gsttaco_ctx*, int code, const std::string& msg) {
    g_last = msg;
    return code;
}

static int g_bad = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

static void check_manifest() {
    Manifest m;
    m.add("net/in/kernel", {6, 3});
    m.add("net/in/bias", {3});
    EXPECT(m.tensors.size() == 2 && m.index.at("net/in/bias") == 1);
    const char* name = nullptr;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = -1;
    EXPECT(m.info(0, &name, shape, &ndim) == 0 && !strcmp(name, "net/in/kernel") && ndim == 2);
    EXPECT(shape[0] == 6 && shape[1] == 3 && shape[2] == 1 && shape[3] == 1);
    EXPECT(m.info(1, nullptr, nullptr, nullptr) == 0);
    EXPECT(m.info(-1, &name, shape, &ndim) == GSTTACO_E_INVALID && m.info(2, &name, shape, &ndim) == GSTTACO_E_INVALID);
    EXPECT(m.first_unloaded() == &m.tensors[0]);

    std::vector<float> w(18), b(3);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)i;
    const int64_t s2[2] = {6, 3}, s1[1] = {3}, wrong_dim[2] = {6, 4}, wrong_rank[3] = {6, 3, 1};
    EXPECT(m.load(nullptr, "net: ", "net/in/kernal", w.data(), s2, 2) == GSTTACO_E_WEIGHTS && g_last == "net: unknown weight 'net/in/kernal'");
    EXPECT(m.load(nullptr, "net: ", "net/in/kernel", w.data(), wrong_rank, 3) == GSTTACO_E_WEIGHTS &&
           g_last == "net: weight 'net/in/kernel' has the wrong shape");
    EXPECT(m.load(nullptr, "", "net/in/kernel", w.data(), wrong_dim, 2) == GSTTACO_E_WEIGHTS && g_last == "weight 'net/in/kernel' has the wrong shape");
    EXPECT(m.load(nullptr, "", "net/in/kernel", w.data(), s1, 1) == GSTTACO_E_WEIGHTS);
    EXPECT(!m.tensors[0].loaded && m.tensors[0].data.empty());            // a refused load leaves the tensor as it was
    EXPECT(m.load(nullptr, "net: ", "net/in/kernel", w.data(), s2, 2) == 0 && m.tensors[0].loaded && m.host("net/in/kernel") == w);
    EXPECT(m.first_unloaded() == &m.tensors[1]);
    w[5] = -1.f;                                                            // a second load of the same tensor: the last copy holds
    EXPECT(m.load(nullptr, "net: ", "net/in/kernel", w.data(), s2, 2) == 0 && m.host("net/in/kernel").size() == 18 && m.host("net/in/kernel")[5] == -1.f);
    EXPECT(m.load(nullptr, "net: ", "net/in/bias", b.data(), s1, 1) == 0 && m.first_unloaded() == nullptr);
}

static uint16_t bf16_bits(float v) {        // to nearest even; the values below are finite
    uint32_t u;
    memcpy(&u, &v, 4);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static void check_packs() {
    const int sizes[] = {1, 15, 16, 17, 33}, taps = 3;
    for (int cin : sizes)
        for (int cout : sizes) {
            std::vector<float> w((size_t)taps * cin * cout);
            for (size_t i = 0; i < w.size(); ++i) w[i] = 0.25f + (float)(i % 251) * 0.03125f;          // finite in bf16 and fp16, never 0
            const int cin_p = (cin + 15) / 16 * 16, n_p = (cout + 15) / 16 * 16, ck = (cin + 31) / 32 * 32;
            EXPECT(voc_pad16(cin) == cin_p && voc_pad16(cout) == n_p);
            std::vector<float> p32((size_t)taps * cin_p * n_p, -7.f);
            voc_pack_f32(w.data(), taps, cin, cout, p32.data());
            EXPECT(gt_hifigan_pack16_words(taps, cin, cout) == (size_t)taps * ck * n_p);
            std::vector<uint16_t> pb((size_t)taps * ck * n_p, 0xffffu), ph(pb);
            EXPECT(gt_hifigan_pack16(w.data(), taps, cin, cout, GT_HG_OP_BF16, pb.data()) == -1);
            EXPECT(gt_hifigan_pack16(w.data(), taps, cin, cout, GT_HG_OP_F16, ph.data()) == -1);
            size_t wrong = 0;
            for (int t = 0; t < taps; ++t)
                for (int k = 0; k < cin_p || k < ck; ++k)
                    for (int n = 0; n < n_p; ++n) {
                        const bool real = k < cin && n < cout;
                        const float v = real ? w[((size_t)t * cin + k) * cout + n] : 0.f;
                        if (k < cin_p) wrong += p32[(((size_t)t * (cin_p / 16) + k / 16) * n_p + n) * 16 + k % 16] != v;
                        const size_t i16 = (((size_t)t * (ck / 32) + k / 32) * n_p + n) * 32 + k % 32;
                        const _Float16 h = (_Float16)v;
                        uint16_t hb;
                        memcpy(&hb, &h, 2);
                        wrong += pb[i16] != (real ? bf16_bits(v) : 0) || ph[i16] != (real ? hb : 0);
                    }
            if (wrong) { printf("pack cin %d cout %d: %zu elements differ from the index formula\n", cin, cout, wrong); ++g_bad; }
        }
    // float16: the first weight that is not finite after rounding is reported by its index
    std::vector<float> w(2 * 17 * 3, 1.f);
    w[40] = 70000.f; w[60] = 1e30f;
    std::vector<uint16_t> p(gt_hifigan_pack16_words(2, 17, 3));
    EXPECT(gt_hifigan_pack16(w.data(), 2, 17, 3, GT_HG_OP_F16, p.data()) == 40);
    EXPECT(gt_hifigan_pack16(w.data(), 2, 17, 3, GT_HG_OP_BF16, p.data()) == -1);
}

int main() {
    check_manifest();
    check_packs();
    printf(g_bad ? "manifest_check: %d checks failed\n" : "manifest_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}

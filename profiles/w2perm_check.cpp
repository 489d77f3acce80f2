// Torch-free check of the side libraries (librrl_hip_w2perm*.so) against the default library THROUGH THE C ABI:
// both are dlopen'ed in one process, fed the same device buffers, and every output is compared byte for byte; then the
// launches are timed with HIP events.  Also run with the parent commit's library as the side library when a clean-up moved a
// surviving kernel's code (the replay draws were added for that, profiles/draw_heads_one_entry_fingerprint.txt).  Starts in milliseconds (no Python, no torch import): written for the last GPU minutes
// of round 3.      hipcc -O2 -o profiles/_ab_w2perm_check profiles/w2perm_check.cpp -ldl
//                  profiles/_ab_w2perm_check recovery_rl_amd/csrc [side library file names ...]
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rrl_hip.h"

typedef int (*fwd_t)(int, int, int, int, int, const float*, int, const float*, const float*, const float*, const float*,
                     const float*, const float*, float*, float*, float*, float*, int, void*);
typedef int (*hid_t)(int, const rrl_hidden_bwd_t*, void*);
typedef int (*gemm_t)(int, int, int, int, int, const float*, int, long long, const float*, int, long long, float*, int,
                      long long, const float*, long long, int, const float*, int, long long, float*, long long, int, void*);
typedef int (*push_t)(const rrl_replay_t*, int64_t, const float*, const float*, const float*, const float*, const float*,
                      const uint8_t*, int32_t*, void*);
typedef int (*sample_t)(const rrl_draw_t*, const rrl_draw_t*, long long, uint64_t, uint64_t, uint64_t*, uint64_t, float*, void*);
typedef int (*sample_packed_t)(int, const rrl_sample_args_t*, void*);

struct Lib {
    std::string name;
    fwd_t fwd;
    hid_t hid_multi;
    gemm_t gemm;
    push_t push;                    // the replay draws (sample_group_kernel / sample_pack_kernel): optional, null in older libraries
    sample_t sample;
    sample_packed_t sample_packed;
    // one stack's hidden-layer backward (dW2 + db2 and dh1) as a launch of its own
    int hid(int G, int B, int H, const float* dh2, const float* h1, const float* W2, float* dW2, float* db2, float* dh1,
            void* stream) const {
        rrl_hidden_bwd_t d{};
        d.G = G; d.B = B; d.H = H;
        d.dh2 = dh2; d.h1 = h1; d.W2 = W2; d.dW2 = dW2; d.db2 = db2; d.dh1 = dh1;
        return hid_multi(1, &d, stream);
    }
};

#define HIP(x)                                                                          \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

static uint64_t lcg = 88172645463325252ULL;
static float rnd() {      // [-1, 1)
    lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
    return float(int32_t(lcg >> 33) - (1 << 30)) / float(1 << 30);
}
struct Buf {
    float* d = nullptr;
    size_t n = 0;
    explicit Buf(size_t n_, float scale = 0.f, bool relu = false) : n(n_) {
        HIP(hipMalloc(&d, n * sizeof(float)));
        std::vector<float> h(n, 0.f);
        if (scale != 0.f)
            for (auto& v : h) {
                v = rnd() * scale;
                if (relu && v < 0.f) v = 0.f;
            }
        HIP(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
    void clear() { HIP(hipMemset(d, 0xff, n * sizeof(float))); }      // NaN pattern: an element nobody wrote shows
    std::vector<float> host() const {
        std::vector<float> h(n);
        HIP(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
        return h;
    }
    ~Buf() { (void)hipFree(d); }
};

static bool load(const std::string& dir, const std::string& file, Lib& lib) {
    const std::string path = dir + "/" + file;
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        printf("cannot load %s: %s\n", path.c_str(), dlerror());
        return false;
    }
    lib.name = file;
    lib.fwd = (fwd_t)dlsym(h, "rrl_mlp3_forward");
    lib.hid_multi = (hid_t)dlsym(h, "rrl_mlp_hidden_backward_multi");
    lib.gemm = (gemm_t)dlsym(h, "rrl_gemm_f32");
    lib.push = (push_t)dlsym(h, "rrl_replay_push");
    lib.sample = (sample_t)dlsym(h, "rrl_sample_multi");
    lib.sample_packed = (sample_packed_t)dlsym(h, "rrl_sample_multi_packed");
    return lib.fwd && lib.hid_multi && lib.gemm;
}

typedef std::vector<std::vector<float>> Result;
static int compare(const char* what, const Lib& lib, const Result& want, const Result& got) {
    int bad = 0;
    for (size_t k = 0; k < want.size(); ++k)
        if (want[k].size() != got[k].size() || memcmp(want[k].data(), got[k].data(), want[k].size() * sizeof(float))) {
            size_t diff = 0, first = 0;
            for (size_t e = 0; e < want[k].size(); ++e)
                if (memcmp(&want[k][e], &got[k][e], 4)) {
                    if (!diff) first = e;
                    ++diff;
                }
            printf("  DIFFERENT %-28s %-34s output %zu: %zu of %zu elements, first at %zu (%g vs %g)\n", lib.name.c_str(), what, k,
                   diff, want[k].size(), first, want[k][first], got[k][first]);
            ++bad;
        }
    if (!bad) printf("  identical %-28s %s\n", lib.name.c_str(), what);
    return bad;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "recovery_rl_amd/csrc";
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        printf("no GPU\n");
        return 3;
    }
    hipDeviceProp_t prop;
    HIP(hipGetDeviceProperties(&prop, 0));
    printf("device: %s (%s), %d CUs\n", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    std::vector<Lib> libs;
    std::vector<std::string> files = {"librrl_hip.so", "librrl_hip_w2perm.so", "librrl_hip_w2perm_all.so", "librrl_hip_w2perm_bwd.so"};
    if (argc > 2) {      // explicit list of side libraries (file names inside <dir>); the default library is always first
        files.resize(1);
        for (int k = 2; k < argc; ++k) files.push_back(argv[k]);
    }
    for (const auto& f : files) {
        Lib l;
        if (load(dir, f, l)) libs.push_back(l);
    }
    if (libs.size() < 2) return 4;
    const int H = 256;
    int bad = 0;
    hipStream_t st;
    HIP(hipStreamCreate(&st));

    // ---- fused stack forward, split path (scratch given) --------------------------------------------------------------
    const int shapes[][4] = {{4096, 4, 1, 2}, {4096, 2, 4, 1}, {2061, 4, 1, 2}, {1040, 2, 4, 1}, {1024, 4, 1, 2}, {256, 4, 1, 2},
                             {256, 2, 4, 1}, {100, 4, 1, 2}};
    for (const auto& s : shapes) {
        const int M = s[0], din = s[1], dout = s[2], G = s[3];
        Buf x(size_t(M) * din, 3.f), W1(size_t(G) * H * din, 1.f), b1(size_t(G) * H, 1.f), W2(size_t(G) * H * H, 1.f / 16),
            b2(size_t(G) * H, 1.f), W3(size_t(G) * dout * H, 1.f / 16), b3(size_t(G) * dout, 1.f);
        Buf h1(size_t(G) * M * H), h2(size_t(G) * M * H), out(size_t(G) * M * dout), scratch(size_t(4) * G * M * dout);
        Result want;
        char what[96];
        snprintf(what, sizeof what, "forward M=%d din=%d dout=%d G=%d", M, din, dout, G);
        for (size_t k = 0; k < libs.size(); ++k) {
            h1.clear(), h2.clear(), out.clear(), scratch.clear();
            const int rc = libs[k].fwd(G, M, H, din, dout, x.d, din, W1.d, b1.d, W2.d, b2.d, W3.d, b3.d, h1.d, h2.d, out.d,
                                       scratch.d, 1, st);
            HIP(hipStreamSynchronize(st));
            if (rc) printf("  %s: rc %d\n", libs[k].name.c_str(), rc), ++bad;
            Result got = {h1.host(), h2.host(), out.host()};
            if (k == 0) {
                want = got;
                size_t nan = 0;
                for (const auto& v : want)
                    for (float e : v) nan += e != e;
                printf("%s: default library wrote %zu NaN (expected 0), out[0] = %g\n", what, nan, want[2][0]);
                bad += nan != 0;
            } else {
                bad += compare(what, libs[k], want, got);
            }
        }
    }
    // ---- hidden layer of the backward (tile form) and the NT GEMM: load_direct operands ---------------------------------
    {
        const int G = 2, B = 256;
        Buf dh2(size_t(G) * B * H, 1.f), h1(size_t(G) * B * H, 1.f, true), W2(size_t(G) * H * H, 1.f / 16);
        Buf dW2(size_t(G) * H * H), db2(size_t(G) * H), dh1(size_t(G) * B * H);
        Buf A(size_t(G) * B * H, 1.f), Bm(size_t(G) * H * H, 1.f / 16), bias(size_t(G) * H, 1.f), C(size_t(G) * B * H);
        Result want_h, want_g;
        for (size_t k = 0; k < libs.size(); ++k) {
            dW2.clear(), db2.clear(), dh1.clear(), C.clear();
            int rc = libs[k].hid(G, B, H, dh2.d, h1.d, W2.d, dW2.d, db2.d, dh1.d, st);
            rc |= libs[k].gemm(0, G, B, H, H, A.d, H, (long long)B * H, Bm.d, H, (long long)H * H, C.d, H, (long long)B * H, bias.d, H,
                               1, nullptr, 0, 0, nullptr, 0, 0, st);
            HIP(hipStreamSynchronize(st));
            if (rc) printf("  %s: rc %d\n", libs[k].name.c_str(), rc), ++bad;
            Result got_h = {dW2.host(), db2.host(), dh1.host()}, got_g = {C.host()};
            if (k == 0) {
                want_h = got_h, want_g = got_g;
                size_t nan = 0;
                for (const auto& v : {want_h[0], want_h[1], want_h[2], want_g[0]})
                    for (float e : v) nan += e != e;
                printf("hidden backward + NT GEMM (G=2, B=256, H=256): default library wrote %zu NaN (expected 0)\n", nan);
                bad += nan != 0;
            } else {
                bad += compare("hidden backward G=2 B=256", libs[k], want_h, got_h);
                bad += compare("gemm NT bias relu 256^3 G=2", libs[k], want_g, got_g);
            }
        }
    }
    // ---- replay draws: every mode of rrl_draw_t with the noise fill, solo (sample_group_kernel) and two seeds packed
    //      (sample_pack_kernel); rings of 32 and of 5 super-chunks (the stratified count scan ends on / inside a lane's run) ----
    for (const int64_t cap : {int64_t(32768), int64_t(5000)}) {
        bool all = true;
        for (const auto& l : libs) all = all && l.push && l.sample && l.sample_packed;
        if (!all) break;
        const int64_t pinned = 1000, rows = cap - pinned - 300;
        const int B = 256, pairs = 3000, n_cnt = int(RRL_POS_CNT_LEN(cap));
        Buf s(2 * rows, 5.f), a(2 * rows, 1.f), r(rows, 1.f), s2(2 * rows, 5.f), m(rows, 1.f);
        {       // r != 0 for every seventh row or so: the stratified classes
            std::vector<float> h = r.host();
            for (auto& v : h) v = v > 0.7f ? 1.f : 0.f;
            HIP(hipMemcpy(r.d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        Buf ring[5] = {Buf(2 * cap), Buf(2 * cap), Buf(cap), Buf(2 * cap), Buf(cap)};
        Buf words(2 * (4 + 6 * 2) + n_cnt);       // state int64[4], six ticks uint64[2] (four draws, two noise fills), pos_cnt
        int64_t* state = (int64_t*)words.d;
        uint64_t *tick = (uint64_t*)(state + 4), *ntick = tick + 8;
        rrl_replay_t rb{ring[0].d, ring[1].d, ring[2].d, ring[3].d, ring[4].d, cap, state, (int32_t*)(ntick + 4),
                        RRL_REPLAY_CLAMP_STRATIFIED, pinned};
        // outputs of two draws (5 tensors, idx int64[B], xu / x2u / xpu) and the normals, for two seeds
        auto outs = [&](std::vector<Buf*>& o) {
            for (int k = 0; k < 2 * 2; ++k)
                for (size_t n : {2 * B, 2 * B, B, 2 * B, B, 2 * B, 4 * B, 4 * B, 4 * B}) o.push_back(new Buf(n));
            o.push_back(new Buf(2 * pairs)), o.push_back(new Buf(2 * pairs));
        };
        std::vector<Buf*> o;
        outs(o);
        auto draw = [&](int k, int mode, int n_pos) {
            Buf** b = &o[9 * k];
            return rrl_draw_t{&rb, mode, n_pos, B - n_pos, 1234 + uint64_t(k), 0, tick + 2 * k, 1, b[0]->d, b[1]->d, b[2]->d, b[3]->d,
                              b[4]->d, (int64_t*)b[5]->d, b[6]->d, b[7]->d, b[8]->d};
        };
        Result want;
        char what[96];
        snprintf(what, sizeof what, "draws cap=%lld solo + 2 seeds packed", (long long)cap);
        for (size_t k = 0; k < libs.size(); ++k) {
            for (auto* b : o) b->clear();
            for (auto& b : ring) HIP(hipMemset(b.d, 0, b.n * sizeof(float)));
            HIP(hipMemset(words.d, 0, words.n * sizeof(float)));
            int rc = libs[k].push(&rb, rows, s.d, a.d, r.d, s2.d, m.d, nullptr, nullptr, st);
            Result got;
            for (int round = 0; round < 2; ++round) {
                // uniform + stratified, demo share + uniform, then both pairs as two seeds of one packed launch
                const rrl_draw_t d[4] = {draw(0, RRL_DRAW_UNIFORM, 0), draw(1, RRL_DRAW_STRATIFIED, 77),
                                         draw(2, RRL_DRAW_DEMO_SHARE, 128), draw(3, RRL_DRAW_UNIFORM, 0)};
                const rrl_sample_args_t args[2] = {{&d[0], &d[1], pairs, 99, 0, ntick, 1, o[36]->d},
                                                   {&d[2], &d[3], pairs, 98, 0, ntick + 2, 1, o[37]->d}};
                for (int pass = 0; pass < 2; ++pass) {
                    if (pass == 0) {
                        rc |= libs[k].sample(&d[0], &d[1], pairs, 99, 0, ntick, 1, o[36]->d, st);
                        rc |= libs[k].sample(&d[2], &d[3], pairs, 98, 0, ntick + 2, 1, o[37]->d, st);
                    } else {
                        rc |= libs[k].sample_packed(2, args, st);
                    }
                    HIP(hipStreamSynchronize(st));
                    for (auto* b : o) got.push_back(b->host());
                    got.push_back(words.host());
                }
            }
            if (rc) printf("  %s: rc %d\n", libs[k].name.c_str(), rc), ++bad;
            if (k == 0) {
                want = got;
                const std::vector<float> w = words.host();
                int64_t st4[4];
                memcpy(st4, w.data(), sizeof st4);
                size_t nan = 0;
                for (float e : got[0]) nan += e != e;
                printf("%s: default library left size %lld, error flag %lld, %zu unwritten floats in the first batch (expected %lld, 0, 0)\n",
                       what, (long long)st4[1], (long long)st4[3], nan, (long long)rows);
                bad += st4[1] != rows || st4[3] != 0 || nan != 0;
            } else {
                bad += compare(what, libs[k], want, got);
            }
        }
        for (auto* b : o) delete b;
    }
    // ---- timing: back-to-back launches on one stream, HIP events; libraries interleaved, three rounds, best of ----------
    {
        hipEvent_t e0, e1;
        HIP(hipEventCreate(&e0));
        HIP(hipEventCreate(&e1));
        const int reps = 300;
        struct Case { const char* name; int M, din, dout, G; } cases[] = {{"forward 4096 rows, 2 heads (Q / Q_risk acting)", 4096, 4, 1, 2},
                                                                        {"forward 4096 rows, 1 head  (policy acting)", 4096, 2, 4, 1},
                                                                        {"forward  256 rows, 2 heads (update batch)", 256, 4, 1, 2}};
        for (const auto& c : cases) {
            Buf x(size_t(c.M) * c.din, 3.f), W1(size_t(c.G) * H * c.din, 1.f), b1(size_t(c.G) * H, 1.f),
                W2(size_t(c.G) * H * H, 1.f / 16), b2(size_t(c.G) * H, 1.f), W3(size_t(c.G) * c.dout * H, 1.f / 16),
                b3(size_t(c.G) * c.dout, 1.f), out(size_t(c.G) * c.M * c.dout), scratch(size_t(4) * c.G * c.M * c.dout);
            std::vector<float> best(libs.size(), 1e30f);
            for (int round = 0; round < 3; ++round)
                for (size_t k = 0; k < libs.size(); ++k) {
                    auto run = [&] {
                        libs[k].fwd(c.G, c.M, H, c.din, c.dout, x.d, c.din, W1.d, b1.d, W2.d, b2.d, W3.d, b3.d, nullptr, nullptr,
                                    out.d, scratch.d, 1, st);
                    };
                    for (int i = 0; i < 20; ++i) run();
                    HIP(hipEventRecord(e0, st));
                    for (int i = 0; i < reps; ++i) run();
                    HIP(hipEventRecord(e1, st));
                    HIP(hipEventSynchronize(e1));
                    float ms = 0.f;
                    HIP(hipEventElapsedTime(&ms, e0, e1));
                    if (ms * 1e3f / reps < best[k]) best[k] = ms * 1e3f / reps;
                }
            printf("%s, us per forward (stack kernel + sum of partials, eager launches):\n", c.name);
            for (size_t k = 0; k < libs.size(); ++k) printf("  %-28s %8.2f\n", libs[k].name.c_str(), best[k]);
        }
        const int G = 2, B = 256;
        Buf dh2(size_t(G) * B * H, 1.f), h1(size_t(G) * B * H, 1.f, true), W2(size_t(G) * H * H, 1.f / 16);
        Buf dW2(size_t(G) * H * H), db2(size_t(G) * H), dh1(size_t(G) * B * H);
        std::vector<float> best(libs.size(), 1e30f);
        for (int round = 0; round < 3; ++round)
            for (size_t k = 0; k < libs.size(); ++k) {
                auto run = [&] { libs[k].hid(G, B, H, dh2.d, h1.d, W2.d, dW2.d, db2.d, dh1.d, st); };
                for (int i = 0; i < 20; ++i) run();
                HIP(hipEventRecord(e0, st));
                for (int i = 0; i < reps; ++i) run();
                HIP(hipEventRecord(e1, st));
                HIP(hipEventSynchronize(e1));
                float ms = 0.f;
                HIP(hipEventElapsedTime(&ms, e0, e1));
                if (ms * 1e3f / reps < best[k]) best[k] = ms * 1e3f / reps;
            }
        printf("hidden-layer backward G=2 B=256 H=256, us per launch (eager launches):\n");
        for (size_t k = 0; k < libs.size(); ++k) printf("  %-28s %8.2f\n", libs[k].name.c_str(), best[k]);
    }
    printf(bad ? "RESULT: %d comparisons DIFFER\n" : "RESULT: every variant equals the default library bit for bit\n", bad);
    return bad ? 1 : 0;
}

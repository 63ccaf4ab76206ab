// kernel_program_fuzz.cpp — boss_kern_create's validation, the host interpreter (boss_kern_eval_host) and the argument checks of the
// batched entry points (boss_kgp_loglike_batch, boss_kgp_fit_batch) over malformed and random programs, as a stand-alone host
// program for a sanitizer build.  No device is touched: only entry points that need none are called.
//
//   hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -w -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -pthread -ldl -o /tmp/kernel_program_fuzz tools/kernel_program_fuzz.cpp boss.jl_amd/csrc/bosship.hip
//   /tmp/kernel_program_fuzz [rounds]
//
// Every program either fails boss_kern_create with BOSS_E_INVALID, or is accepted and then evaluated at 16 point pairs (whatever the
// values: NaN and Inf are results).  Exit status 0 and the sanitizers' silence are the result; the counts are printed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/bosship.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static int rnd_int(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

static long n_ok = 0, n_bad = 0;

// The batched entry points over an accepted program, as far as they go without a device: every call here is decided by the argument
// checks in front of the device context (NULL program, another x_dim, S < 0, NULL arrays with S > 0 -> BOSS_E_INVALID; S = 0 -> BOSS_OK
// with nothing written).  X doubles as the hyper-parameter arrays: it is never read.
static void batch_refusals(const boss_kern_t* k, int d, const double* X, double* out) {
    boss_gp_t* hs[3] = {nullptr, nullptr, nullptr};
    int st[3] = {0, 0, 0};
    const int S = rnd_int(1, 3), N = rnd_int(1, 16);
    struct Case { const boss_kern_t* k; int d, S; const double *X, *y, *lam, *amp, *sig; int want; };
    const Case cases[] = {
        {nullptr, d, S, X, X, X, X, X, BOSS_E_INVALID},     {k, d + 1, S, X, X, X, X, X, BOSS_E_INVALID},
        {k, d, -rnd_int(1, 5), X, X, X, X, X, BOSS_E_INVALID}, {k, d, S, nullptr, X, X, X, X, BOSS_E_INVALID},
        {k, d, S, X, nullptr, X, X, X, BOSS_E_INVALID},      {k, d, S, X, X, nullptr, X, X, BOSS_E_INVALID},
        {k, d, S, X, X, X, nullptr, X, BOSS_E_INVALID},      {k, d, S, X, X, X, X, nullptr, BOSS_E_INVALID},
        {k, d, 0, X, X, nullptr, nullptr, nullptr, BOSS_OK},
    };
    for (const Case& c : cases) {
        const int a = boss_kgp_loglike_batch(0, c.d, N, c.X, c.y, nullptr, c.k, c.S, c.lam, c.amp, c.sig, nullptr, 0, out, st);
        const int b = boss_kgp_fit_batch(0, c.k, c.d, N, c.X, c.y, nullptr, 0, nullptr, c.S, c.lam, c.amp, c.sig, hs, out, st);
        if (a != c.want || b != c.want || hs[0] || hs[1] || hs[2]) {
            std::fprintf(stderr, "batched entry points: status %d / %d, expected %d (%s)\n", a, b, c.want, boss_last_error());
            std::exit(7);
        }
    }
    if (boss_kgp_loglike_batch(0, d, N, X, X, nullptr, k, S, X, X, X, nullptr, 0, nullptr, st) != BOSS_E_INVALID ||
        boss_kgp_fit_batch(0, k, d, N, X, X, nullptr, 0, nullptr, S, X, X, X, nullptr, out, st) != BOSS_E_INVALID)
        std::exit(7);
}

static int try_program(int d, int nc, const double* consts, int ni, const int* code, int out_id) {
    boss_kern_t* k = nullptr;
    const int rc = boss_kern_create(d, nc, consts, ni, code, out_id, &k);
    if (rc != BOSS_OK) {
        if (rc != BOSS_E_INVALID || k != nullptr) {
            std::fprintf(stderr, "unexpected status %d (%s)\n", rc, boss_last_error());
            std::exit(2);
        }
        ++n_bad;
        return rc;
    }
    ++n_ok;
    const int n = 16;
    std::vector<double> U((size_t)d * n), V((size_t)d * n), out(n);
    for (auto& x : U) x = (double)rnd_int(-3000, 3000) / 1000.0;
    for (auto& x : V) x = (double)rnd_int(-3000, 3000) / 1000.0;
    if (boss_kern_eval_host(k, n, U.data(), V.data(), out.data()) != BOSS_OK) std::exit(3);
    if (boss_kern_eval_host(k, 0, nullptr, nullptr, nullptr) != BOSS_OK) std::exit(3);
    batch_refusals(k, d, U.data(), out.data());
    boss_kern_free(k);
    return rc;
}

int main(int argc, char** argv) {
    const long rounds = argc > 1 ? std::atol(argv[1]) : 200000;
    // hand-made edge cases first
    {
        const int mul01[3] = {2, 0, 1};
        try_program(1, 0, nullptr, 1, mul01, 2);                       // u0 * v0
        try_program(0, 0, nullptr, 0, nullptr, 0);
        try_program(17, 0, nullptr, 0, nullptr, 0);
        try_program(-1, 0, nullptr, 0, nullptr, 0);
        try_program(1, -1, nullptr, 0, nullptr, 0);
        try_program(1, 33, nullptr, 0, nullptr, 0);
        try_program(1, 1, nullptr, 0, nullptr, 0);                     // constants announced, none given
        try_program(1, 0, nullptr, 65, mul01, 2);
        try_program(1, 0, nullptr, -5, mul01, 2);
        try_program(1, 0, nullptr, 1, nullptr, 2);
        try_program(1, 0, nullptr, 1, mul01, 3);
        try_program(1, 0, nullptr, 1, mul01, -1);
        try_program(1, 0, nullptr, 1, mul01, 1 << 30);
        const int self[3] = {2, 2, 0}, fwd[3] = {2, 0, 99}, neg[3] = {2, -7, 0}, op[3] = {-1, 0, 1}, op2[3] = {1 << 20, 0, 1}, un[3] = {4, 0, 1};
        for (const int* c : {self, fwd, neg, op, op2, un}) try_program(1, 0, nullptr, 1, c, 2);
        if (boss_kern_create(1, 0, nullptr, 0, nullptr, 0, nullptr) != BOSS_E_INVALID) return 4;
        if (boss_kern_eval_host(nullptr, 1, nullptr, nullptr, nullptr) != BOSS_E_INVALID) return 4;
        boss_kern_free(nullptr);
        // the longest program: 16 dimensions, 32 constants, 64 instructions, every id in range
        std::vector<double> c32(32, 0.5);
        std::vector<int> code(3 * 64);
        for (int i = 0; i < 64; ++i) {
            code[3 * i] = i % 4;                                        // ADD SUB MUL DIV
            code[3 * i + 1] = i;                                        // the 32 inputs, then the 32 constants
            code[3 * i + 2] = i == 0 ? 1 : 64 + i - 1;
        }
        if (try_program(16, 32, c32.data(), 64, code.data(), 64 + 63) != BOSS_OK) return 5;
    }
    // random programs: ids, opcodes and sizes drawn a little beyond their valid ranges
    for (long r = 0; r < rounds; ++r) {
        const int d = rnd_int(-1, 18), nc = rnd_int(-1, 34), ni = rnd_int(-1, 66);
        std::vector<double> consts(nc > 0 ? nc : 0);
        for (auto& x : consts) {
            const int k = rnd_int(0, 40);
            x = k == 0 ? NAN : k == 1 ? INFINITY : (double)rnd_int(-5000, 5000) / 1000.0;
        }
        std::vector<int> code(ni > 0 ? 3 * ni : 0);
        const int base = 2 * (d > 0 ? d : 0) + (nc > 0 ? nc : 0);
        const bool tidy = rnd_int(0, 3) != 0;                            // mostly well-formed, so that many programs are evaluated
        for (int i = 0; i < ni; ++i) {
            const int opc = tidy ? rnd_int(0, 15) : rnd_int(-2, 18);
            const bool unary = opc >= 4 && opc <= 12;
            const int top = base + i;
            code[3 * i] = opc;
            code[3 * i + 1] = tidy && top > 0 ? rnd_int(0, top - 1) : rnd_int(-2, top + 2);
            code[3 * i + 2] = unary ? (tidy ? -1 : rnd_int(-2, 1)) : (tidy && top > 0 ? rnd_int(0, top - 1) : rnd_int(-2, top + 2));
        }
        const int nval = base + (ni > 0 ? ni : 0);
        const int out_id = tidy && nval > 0 ? rnd_int(0, nval - 1) : rnd_int(-2, nval + 2);
        try_program(d, nc, consts.empty() ? nullptr : consts.data(), ni, code.empty() ? nullptr : code.data(), out_id);
    }
    std::printf("kernel_program_fuzz: %ld programs accepted and evaluated, %ld refused\n", n_ok, n_bad);
    return n_ok > 0 && n_bad > 0 ? 0 : 6;
}

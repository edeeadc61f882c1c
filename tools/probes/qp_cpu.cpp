// One CPU thread running the coordinate pass of include/pbd.h's "Training QP" contract (plain updates only: one id per entry,
// no fixed set) on a synthetic cache of the person model's shape (77 blocks, 20 928 values per entry), with the header's
// reduction R (1024 lane partials, then the halving trees).  Prints one JSON line: microseconds per step.  A yardstick for
// k_qp_pass, not a product path.
//     g++ -O2 -std=c++17 -o qp_cpu tools/probes/qp_cpu.cpp && ./qp_cpu [entries]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

static double R(const double *p, int n)
{
    double lane[1024] = {0};
    for (int j = 0; j < n; ++j) lane[j & 1023] = lane[j & 1023] + p[j];
    for (int g = 0; g < 16; ++g)
        for (int h = 32; h >= 1; h >>= 1)
            for (int l = 0; l < h; ++l) lane[64 * g + l] = lane[64 * g + l] + lane[64 * g + l + h];
    double t[16];
    for (int g = 0; g < 16; ++g) t[g] = lane[64 * g];
    for (int h = 8; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l) t[l] = t[l] + t[l + h];
    return t[0];
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 4000;
    const int nb = 77, L = 126301, V = 20928;
    std::vector<int> off(nb), len(nb), st(nb);
    int pos = 0, coord = 0;
    for (int b = 0; b < nb; ++b) {   // 26 biases, 25 deformations, 26 filters of 800
        len[b] = b < 26 ? 1 : b < 51 ? 4 : 800;
        if (b == 26) coord = 2000;
        off[b] = coord; st[b] = pos;
        coord += len[b] * 3; pos += len[b];
    }
    if (pos > V || coord > L) return 1;
    std::vector<float> x((size_t)n * V);
    uint64_t s = 12345;
    for (auto &v : x) { s = s * 6364136223846793005ULL + 1442695040888963407ULL; v = (float)((double)(s >> 40) / (1 << 24) - 0.5) * 4e-4f; }
    std::vector<double> b(n, 0.002), d(n), a(n, 0.0), w(L, 0.0), p(V);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < pos; ++j) p[j] = (double)x[(size_t)i * V + j] * (double)x[(size_t)i * V + j];
        d[i] = R(p.data(), pos);
    }
    std::vector<int> cmap(pos);
    for (int bb = 0; bb < nb; ++bb) for (int k = 0; k < len[bb]; ++k) cmap[st[bb] + k] = off[bb] + k;
    const auto t0 = std::chrono::steady_clock::now();
    double loss = 0;
    for (int i = 0; i < n; ++i) {
        const float *xi = &x[(size_t)i * V];
        for (int j = 0; j < pos; ++j) p[j] = w[cmap[j]] * (double)xi[j];
        const double G = R(p.data(), pos) - b[i];
        loss = loss + (-G > 0 ? -G : 0);
        const double Ai = a[i];
        if (!((Ai == 0 && G >= 0) || (Ai >= 1 && G <= 0))) {
            double an = Ai - G / d[i];
            an = an < 0 ? 0 : an;
            an = an > 1 ? 1 : an;
            const double dA = an - Ai;
            a[i] = an;
            for (int j = 0; j < pos; ++j) w[cmap[j]] = w[cmap[j]] + dA * (double)xi[j];
            for (int k = 0; k < 25; ++k) { double &v = w[off[26 + k]]; v = v < 0 ? 0 : v; double &u = w[off[26 + k] + 2]; u = u < 0 ? 0 : u; }
        }
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"cpu_one_thread\": true, \"steps\": %d, \"values\": %d, \"us_per_step\": %.3f, \"loss\": %.6g}\n", n, pos, us / n, loss);
    return 0;
}

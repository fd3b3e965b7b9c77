// Host-only run of the bodies of csrc/spdfgto.hip (they are __host__ __device__), meant for a sanitizer build before the
// first run on a device: every element of a small molecule is computed on the CPU by the code the kernels run -- the
// host description (gto_describe, SpdfRoute::tag and its sorted order), the pair table, the one-electron body, the
// two-electron bodies of every class the molecule has through the class switch, with and without the gradient, full and
// packed forms, the dipole body and the dipole-gradient body -- and held against the arrays of the host statement
// gto_spdf.spdf_gaussian_mol, which tools/micro/spdfgto_cpu_check.py writes into a file.  It also checks that the sorted
// ket order gives every packed pair exactly one owner.  No device is touched.
//   python tools/micro/spdfgto_cpu_check.py /tmp/spdf_case        (writes /tmp/spdf_case.<name>.bin per molecule)
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Ievcont_amd/csrc \
//         tools/micro/spdfgto_cpu_check.hip -fsanitize=address,undefined -o spdfgto_cpu_check
//   ./spdfgto_cpu_check /tmp/spdf_case.small_f.bin /tmp/spdf_case.df_atom.bin
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../evcont_amd/csrc/spdfgto.hip"

namespace evc {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace evc

static const double kGate = 1e-10;   // the project's gate of the device against the host statement
static int g_failed = 0;

static std::vector<double> read_doubles(FILE *f, size_t n) {
    std::vector<double> v(n);
    if (fread(v.data(), sizeof(double), n, f) != n) {
        printf("FAILED short file\n");
        exit(2);
    }
    return v;
}
static std::vector<int> read_ints(FILE *f, size_t n) {
    std::vector<int> v(n);
    if (fread(v.data(), sizeof(int), n, f) != n) {
        printf("FAILED short file\n");
        exit(2);
    }
    return v;
}

// max |x - ref| / max(1, max |ref|)
static void compare(const char *file, const char *what, const std::vector<double> &x, const std::vector<double> &ref) {
    double d = 0.0, m = 1.0;
    bool nan = x.size() != ref.size();
    for (size_t i = 0; i < ref.size() && !nan; ++i) {
        if (x[i] != x[i]) nan = true;
        d = fmax(d, fabs(x[i] - ref[i]));
        m = fmax(m, fabs(ref[i]));
    }
    printf("%s %-22s %.2e%s\n", file, what, d / m, nan ? " NaN or size" : "");
    if (nan || !(d / m < kGate)) {
        printf("FAILED %s %s\n", file, what);
        ++g_failed;
    }
}

static std::vector<double> poisoned(size_t n) { return std::vector<double>(n, NAN); }

static void check(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        printf("FAILED cannot open %s\n", path);
        exit(2);
    }
    const std::vector<int> hd = read_ints(f, 4);
    const int natm = hd[0], nshell = hd[1], nprim = hd[2], N = hd[3];
    const std::vector<int> sa = read_ints(f, nshell), sl = read_ints(f, nshell), so = read_ints(f, nshell + 1);
    const std::vector<double> ex = read_doubles(f, nprim), co = read_doubles(f, nprim), R = read_doubles(f, natm * 3),
                              Z = read_doubles(f, natm), O = read_doubles(f, 3);
    const size_t n2 = (size_t)N * N, n4 = n2 * n2, Ms = (size_t)N * (N + 1) / 2;
    const std::vector<double> rS = read_doubles(f, n2), rH = read_doubles(f, n2), rIp = read_doubles(f, 3 * n2),
                              rDh = read_doubles(f, natm * 3 * n2), rEri = read_doubles(f, n4),
                              rIp1 = read_doubles(f, 3 * n4), rDip = read_doubles(f, 3 * n2),
                              rIpdip = read_doubles(f, 9 * n2);
    fclose(f);

    SpdfPrims bs;
    SpdfAos ao;
    int np = 0, nao = 0;
    if (gto_describe<SpdfRoute>("spdfgto_cpu_check", natm, nshell, 1, sa.data(), sl.data(), so.data(), ex.data(), co.data(),
                                bs, ao, np, nao) || np != nprim || nao != N) {
        printf("FAILED %s: gto_describe\n", path);
        ++g_failed;
        return;
    }
    // the sorted order: a permutation of the functions, ascending in l, and every packed pair owned once
    {
        std::vector<int> seen(N, 0), owner(Ms, 0);
        bool ok = true;
        for (int i = 0; i < N; ++i) {
            ok = ok && ao.perm[i] < N && ++seen[ao.perm[i]] == 1;
            if (i && ok) ok = spdf_l(ao.kind[ao.perm[i - 1]]) <= spdf_l(ao.kind[ao.perm[i]]);
        }
        for (int vs = 0; vs < (int)Ms && ok; ++vs) {
            const int ra = gto_tri_row(vs), rb = vs - ra * (ra + 1) / 2, fa = ao.perm[ra], fb = ao.perm[rb];
            const int kap = fa > fb ? fa : fb, lam = fa > fb ? fb : fa;
            ok = ++owner[kap * (kap + 1) / 2 + lam] == 1;
        }
        if (!ok) {
            printf("FAILED %s: sorted ket order\n", path);
            ++g_failed;
            return;
        }
    }
    std::vector<double> tab((size_t)nprim * nprim * kGtoRow);
    for (int i = 0; i < nprim * nprim; ++i) gto_pair_body(i, 0, bs, R.data(), natm, nprim, tab.data());

    // one-electron arrays, with and without the gradient
    std::vector<double> S = poisoned(n2), H = poisoned(n2), Ip = poisoned(3 * n2), Dh = poisoned(natm * 3 * n2);
    for (int e = 0; e < (int)Ms; ++e)
        spdf_one_body<true>(e, 0, ao, tab.data(), R.data(), Z.data(), N, natm, nprim, S.data(), H.data(), Ip.data(),
                            Dh.data());
    compare(path, "S", S, rS);
    compare(path, "hcore", H, rH);
    compare(path, "ipovlp", Ip, rIp);
    compare(path, "dhcore", Dh, rDh);
    S = poisoned(n2);
    H = poisoned(n2);
    for (int e = 0; e < (int)Ms; ++e)
        spdf_one_body<false>(e, 0, ao, tab.data(), R.data(), Z.data(), N, natm, nprim, S.data(), H.data(), nullptr, nullptr);
    compare(path, "S energy-only", S, rS);
    compare(path, "hcore energy-only", H, rH);

    // two-electron arrays: full forms with the gradient, packed forms with it, full form without it
    std::vector<double> eri = poisoned(n4), ip1 = poisoned(3 * n4);
    for (int by = 0; by < (int)n2; ++by)
        for (int vs = 0; vs < (int)Ms; ++vs)
            spdf_two<true>(by / N, by % N, vs, 0, ao, tab.data(), N, nprim, 0, 0, eri.data(), ip1.data());
    compare(path, "eri", eri, rEri);
    compare(path, "eri_ip1", ip1, rIp1);
    std::vector<double> e4 = poisoned(Ms * Ms), i2 = poisoned(3 * n2 * Ms);
    for (int by = 0; by < (int)n2; ++by)
        for (int vs = 0; vs < (int)Ms; ++vs)
            spdf_two<true>(by / N, by % N, vs, 0, ao, tab.data(), N, nprim, 1, 1, e4.data(), i2.data());
    {
        bool same = true;
        for (int m = 0; m < N && same; ++m)
            for (int n = 0; n <= m && same; ++n)
                for (int k = 0; k < N && same; ++k)
                    for (int l = 0; l <= k && same; ++l)
                        same = e4[((size_t)m * (m + 1) / 2 + n) * Ms + k * (k + 1) / 2 + l] == eri[((size_t)m * N + n) * n2 + k * N + l];
        for (size_t row = 0; row < 3 * n2 && same; ++row)
            for (int k = 0; k < N && same; ++k)
                for (int l = 0; l <= k && same; ++l) same = i2[row * Ms + k * (k + 1) / 2 + l] == ip1[row * n2 + k * N + l];
        printf("%s packed forms are the full forms, packed: %s\n", path, same ? "yes" : "NO");
        if (!same) ++g_failed;
    }
    eri = poisoned(n4);
    for (int by = 0; by < (int)Ms; ++by) {
        const int mu = gto_tri_row(by), nu = by - mu * (mu + 1) / 2;
        for (int vs = 0; vs < (int)Ms; ++vs)
            spdf_two<false>(mu, nu, vs, 0, ao, tab.data(), N, nprim, 0, 0, eri.data(), nullptr);
    }
    compare(path, "eri energy-only", eri, rEri);

    // dipole integrals and their gradient
    std::vector<double> dip = poisoned(3 * n2), ipdip = poisoned(9 * n2);
    for (int e = 0; e < (int)Ms; ++e) spdf_dipole_body(e, 0, bs, ao, R.data(), N, natm, O[0], O[1], O[2], dip.data());
    for (int i = 0; i < (int)n2; ++i) spdf_dipole_grad_body(i, 0, bs, ao, R.data(), N, natm, O[0], O[1], O[2], ipdip.data());
    compare(path, "dip", dip, rDip);
    compare(path, "ipdip", ipdip, rIpdip);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: spdfgto_cpu_check case.bin ...\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) check(argv[i]);
    if (g_failed) return 1;
    printf("OK\n");
    return 0;
}

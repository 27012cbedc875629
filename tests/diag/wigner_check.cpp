// wigner_check.cpp — csrc/qcart_wigner.hpp as a plain C++ program (tests/test_wigner_cpu.py builds it with g++ and
// AddressSanitizer + UBSan): reads "x_n h P" and P momenta (C99 hex floats, or nan / inf) from the file named by
// argv[1] and prints the table, one line per lag k = 1 .. (x_n - 1) / 2 with "cos sin" of every momentum, as hex
// floats. A refused call prints "refused: <text>" and exits with 2; the output buffer is allocated at its exact size,
// so a write past the table is a sanitizer error.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../deepreinforcementlearningcontrolofquantumcartpoles_amd/csrc/qcart_wigner.hpp"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: wigner_check SCRIPT\n");
        return 64;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 66;
    }
    long x_n = 0, P = 0;
    char word[64];
    if (std::fscanf(f, "%ld %63s %ld", &x_n, word, &P) != 3 || P < 0 || P > 100000) {
        std::fprintf(stderr, "bad script header\n");
        return 65;
    }
    const double h = std::strtod(word, nullptr);
    std::vector<double> p((size_t)P);
    for (long j = 0; j < P; ++j) {
        if (std::fscanf(f, "%63s", word) != 1) {
            std::fprintf(stderr, "bad script: p[%ld]\n", j);
            return 65;
        }
        p[(size_t)j] = std::strtod(word, nullptr);
    }
    std::fclose(f);
    const bool sized = x_n >= 1 && x_n <= qcart::wigner::kMaxPoints && P >= 1 && P <= qcart::wigner::kMaxMomenta;
    const long rows = sized ? qcart::wigner::table_rows((int32_t)x_n) : 0;
    std::vector<double> out(rows > 0 ? (size_t)rows * (size_t)P * 2 : 1);
    const char* why = nullptr;
    const int rc = qcart::wigner::qc_wigner_build_table((int32_t)x_n, h, p.empty() ? nullptr : p.data(), (int32_t)P,
                                                        out.data(), &why);
    if (rc != QC_OK) {
        std::printf("refused: %s\n", why ? why : "?");
        return rc == QC_EINVAL ? 2 : 3;
    }
    if (why != nullptr) return 4;
    for (long k = 0; k < rows; ++k) {
        for (long j = 0; j < 2 * P; ++j) std::printf("%a ", out[(size_t)(k * 2 * P + j)]);
        std::printf("\n");
    }
    return 0;
}

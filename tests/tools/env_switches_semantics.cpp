// Host-only check of csrc/env_switches.h (its own main; no HIP, no library): for every parsing rule the library's getenv lines spelled
// by hand before the table existed, the old expression against the accessor that replaced it, on unset, empty, non-numeric, zero,
// negative, fractional, padded and extreme values; then the latch of once<id>().  Exit status 0 and "0 mismatches" when they agree.
// Built and run by tests/test_env_switches.py:  c++ -std=c++17 -I columbiaimagesearch_amd/csrc env_switches_semantics.cpp
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include "env_switches.h"

static int bad = 0;
static const char* v = nullptr;
#define CHECK(a, b) do { if ((a) != (b)) { printf("MISMATCH line %d value '%s'\n", __LINE__, v ? v : "(unset)"); bad++; } } while (0)

int main() {
    const char* vals[] = {nullptr, "", "abc", "0", "1", "-3", "16", "64", "2", "4.75", "1e3", " 7", "2147483647", "-2147483648", "99999", "4294967296", "8589934597"};
    const char* names[] = {"CIS_S4_FRAC", "CIS_SEG_MAX", "CIS_S4_PER_CU", "CIS_CNN_GRAPH", "CIS_NO_TINY", "CIS_S4_ZL", "CIS_S4_ZS", "CIS_PCA_BK", "CIS_PCA_PF", "CIS_FINE",
                           "CIS_STREAM_GRID", "CIS_TINY_MIN_QUOTA", "CIS_SCAN3_TWOPASS", "CIS_REMOVE_LDS_MAX", "CIS_WORKSPACE_GB", "CIS_COARSE", "CIS_CNN_POISON",
                           "CIS_STREAM_SS", "CIS_STREAM_K", "CIS_CNN_SPLIT_TARGET", "CIS_STREAM_CHUNK"};
    for (const char* val : vals) {
        v = val;
        for (const char* n : names) { if (v) setenv(n, v, 1); else unsetenv(n); }
        // INT with the table's default, into an int
        { const int o = getenv("CIS_S4_FRAC") ? atoi(getenv("CIS_S4_FRAC")) : 8; const int w = envsw::call<envsw::s4_frac>(); CHECK(o, w); }
        { const int o = getenv("CIS_COARSE") ? atoi(getenv("CIS_COARSE")) : -1; const int w = envsw::call<envsw::coarse>(); CHECK(o, w); }
        { const char* e = getenv("CIS_CNN_POISON"); const int o = e ? atoi(e) : 0; const int w = envsw::call<envsw::cnn_poison>(); CHECK(o, w); }
        // ... compared or widened directly: through (int), as atoi gave it
        { const bool o = !(getenv("CIS_PCA_PF") && atoi(getenv("CIS_PCA_PF")) == 0); CHECK(o, (int)envsw::call<envsw::pca_pf>() != 0); }
        { const bool o = !(getenv("CIS_FINE") && atoi(getenv("CIS_FINE")) == 0); CHECK(o, (int)envsw::call<envsw::fine>() != 0); }
        { const char* te = getenv("CIS_CNN_SPLIT_TARGET"); const int64_t o = te ? atoi(te) : 512; const int64_t w = (int)envsw::call<envsw::cnn_split_target>(); CHECK(o, w); }
        // ... into 64 bits (atoll)
        { const int64_t o = getenv("CIS_TINY_MIN_QUOTA") ? atoll(getenv("CIS_TINY_MIN_QUOTA")) : 8192; const int64_t w = envsw::call<envsw::tiny_min_quota>(); CHECK(o, w); }
        // INT with the site's default
        { int o = 1, w = 1; if (const char* e = getenv("CIS_SCAN3_TWOPASS")) o = atoi(e); w = envsw::call<envsw::scan3_twopass>(w); CHECK(o, w); }
        { const char* e = getenv("CIS_REMOVE_LDS_MAX"); const int o = e ? atoi(e) : 1024; const int w = envsw::call<envsw::remove_lds_max>((int)1024); CHECK(o, w); }
        for (int big = 0; big < 2; ++big) { const bool o = getenv("CIS_PCA_BK") ? atoi(getenv("CIS_PCA_BK")) == 16 : big; const bool w = envsw::call<envsw::pca_bk>(big ? 16 : 32) == 16; CHECK(o, w); }
        for (int force = 0; force < 2; ++force) {  // CIS_STREAM_SS: "set at all, then atoll", only under scan mode 6; CIS_STREAM_K only with it
            int64_t ss = 8, kth = 9, ss2 = 8, kth2 = 9;
            if (force && getenv("CIS_STREAM_SS")) { ss = atoll(getenv("CIS_STREAM_SS")); kth = getenv("CIS_STREAM_K") ? atoll(getenv("CIS_STREAM_K")) : kth; }
            const int64_t se = force ? envsw::call<envsw::stream_ss>(INT64_MIN) : INT64_MIN;
            if (se != INT64_MIN) { ss2 = se; kth2 = envsw::call<envsw::stream_k>(kth2); }
            CHECK(ss, ss2); CHECK(kth, kth2);
        }
        // INT_POS
        { int o = 4096, w = 4096; if (const char* e = getenv("CIS_SEG_MAX")) o = atoi(e) > 0 ? atoi(e) : o; w = envsw::call<envsw::seg_max>(w); CHECK(o, w); }
        { int o = 5, w = 5; if (const char* e = getenv("CIS_S4_PER_CU")) o = atoi(e) > 0 && atoi(e) < o ? atoi(e) : o; w = std::min(w, envsw::call<envsw::s4_per_cu>(w)); CHECK(o, w); }
        { int64_t o = 512, w = 512; if (const char* e = getenv("CIS_STREAM_GRID")) o = atoll(e) > 0 ? atoll(e) : o; w = envsw::call<envsw::stream_grid>(w); CHECK(o, w); }
        { int64_t o = 65536, w = 65536; if (const char* e = getenv("CIS_STREAM_CHUNK")) o = atoi(e) > 0 ? atoi(e) : o; w = envsw::call<envsw::stream_chunk>((int)w); CHECK(o, w); }
        // NONZERO, PRESENT
        { const char* ge = getenv("CIS_CNN_GRAPH"); const bool o = ge && atoi(ge) != 0; CHECK(o, envsw::call<envsw::cnn_graph>()); }
        { CHECK(getenv("CIS_NO_TINY") != nullptr, envsw::call<envsw::no_tiny>()); }
        // REAL: the table's default, the site's default
        { const float o = getenv("CIS_S4_ZL") ? (float)atof(getenv("CIS_S4_ZL")) : 4.5f; const float w = (float)envsw::call<envsw::s4_zl>(); CHECK(o, w); }
        { const float o = getenv("CIS_S4_ZS") ? (float)atof(getenv("CIS_S4_ZS")) : 4.0f; const float w = envsw::call<envsw::s4_zs>(4.0f); CHECK(o, w); }
        { const double o = (getenv("CIS_WORKSPACE_GB") ? atof(getenv("CIS_WORKSPACE_GB")) : 24.0) * 1.0e9; const double w = envsw::call<envsw::workspace_gb>() * 1.0e9; CHECK(o, w); }
    }
    // LATCHED: the value of the first use stays, and another switch latches on its own first use, not on the first use of any
    v = "latch";
    setenv("CIS_FORCE_SCAN", "3", 1);
    const int a = envsw::once<envsw::force_scan>();
    setenv("CIS_FORCE_SCAN", "2", 1);
    setenv("CIS_SCAN_LONG", "0", 1);
    CHECK(a, 3);
    CHECK((int)envsw::once<envsw::force_scan>(), 3);
    CHECK((int)envsw::once<envsw::scan_long>(), 0);
    printf("%d mismatches, %d switches\n", bad, (int)envsw::n_switches);
    return bad != 0;
}

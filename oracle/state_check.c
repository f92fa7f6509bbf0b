/* oracle/state_check.c — TEST INFRASTRUCTURE ONLY.
 *
 * A stand-alone run of the oracle's state accessors (fxo_clone, fxo_set_tram, fxo_set_cursors) for a build under
 * AddressSanitizer + UndefinedBehaviorSanitizer (oracle/Makefile `state_check`; tests/test_oracle_state.py runs it):
 * run, clone, write a window into both, carry on with both, compare everything, free everything.
 * Exit status 0 and "state_check ok" when every comparison held.
 */
#include "fx8010_oracle.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char* PROGRAM =
    "input in 0\n"
    "output out 0\n"
    "control c = 0.3\n"
    "static noise\n"
    "itramsize 11 \n"
    "xtramsize 23 \n"
    "static a\n"
    "static b\n"
    "static d\n"
    "idelay read, a, at, 0\n"
    "xdelay read, b, at, 0\n"
    "macs d, a, b, c\n"
    "macs d, d, noise, 0.25\n"
    "skip ccr, ccr, 8, 1\n"
    "macs d, d, in, 0.5\n"
    "idelay write, d, at, 0\n"
    "xdelay write, in, at, 0\n"
    "macs out, d, in, 0.5\n"
    "end\n";

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "state_check: line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static float input_at(int t) { return (float)((t * 37) % 101 - 50) / 64.0f; }

static void run(fxo_t* f, int t0, int n, float* out) {
    for (int t = 0; t < n; ++t) {
        float in = input_at(t0 + t);
        fxo_process(f, &in, out + t);
    }
}

static int same_state(fxo_t* a, fxo_t* b) {
    static float ta[64], tb[64];
    int ca[4], cb[4];
    int32_t la[2], lb[2];
    int ok = 1;
    for (int which = 0; which < 2; ++which) {
        ok &= fxo_tram(a, which, ta, 64) == 64 && fxo_tram(b, which, tb, 64) == 64 && memcmp(ta, tb, sizeof ta) == 0;
    }
    fxo_cursors(a, ca); fxo_cursors(b, cb);
    fxo_lfsr(a, la); fxo_lfsr(b, lb);
    ok &= memcmp(ca, cb, sizeof ca) == 0 && memcmp(la, lb, sizeof la) == 0;
    ok &= fxo_instruction_counter(a) == fxo_instruction_counter(b) && fxo_ood_flags(a) == fxo_ood_flags(b);
    ok &= fxo_num_registers(a) == fxo_num_registers(b);
    for (int i = 0; ok && i < fxo_num_registers(a); ++i) {
        float va = fxo_register_value(a, i), vb = fxo_register_value(b, i);
        ok &= memcmp(&va, &vb, 4) == 0 && strcmp(fxo_register_name(a, i), fxo_register_name(b, i)) == 0;
    }
    return ok;
}

int main(void) {
    fxo_t* f = fxo_create(1);
    CHECK(fxo_load_text(f, PROGRAM));
    float ya[64], yb[64];
    run(f, 0, 29, ya);

    fxo_t* g = fxo_clone(f);
    CHECK(g != NULL && same_state(f, g));
    CHECK(fxo_clone(NULL) == NULL);

    /* a window of bit patterns, a quiet NaN with a payload among them, into both; the ends of the arrays; refusals */
    uint32_t bits[5] = { 0x3f000000u, 0x7fc12345u, 0x80000000u, 0x00000001u, 0xbe800000u };
    float words[5], back[16];
    memcpy(words, bits, sizeof words);
    for (int which = 0; which < 2; ++which) {
        CHECK(fxo_set_tram(f, which, 3, words, 5) == 5);
        CHECK(fxo_set_tram(g, which, 3, words, 5) == 5);
        CHECK(fxo_tram(g, which, back, 8) == 8 && memcmp(back + 3, words, sizeof words) == 0);
    }
    CHECK(fxo_set_tram(f, 0, 8192 - 5, words, 5) == 5);
    CHECK(fxo_set_tram(g, 0, 8192 - 5, words, 5) == 5);
    CHECK(fxo_set_tram(f, 1, 1048576 - 5, words, 5) == 5);
    CHECK(fxo_set_tram(g, 1, 1048576 - 5, words, 5) == 5);
    CHECK(fxo_set_tram(f, 0, 8192 - 4, words, 5) == 0);
    CHECK(fxo_set_tram(f, 1, 1048576 - 4, words, 5) == 0);
    CHECK(fxo_set_tram(f, 0, -1, words, 5) == 0);
    CHECK(fxo_set_tram(f, 2, 0, words, 5) == 0);
    CHECK(fxo_set_tram(f, 0, 0, words, -1) == 0);
    CHECK(fxo_set_tram(f, 0, 8192, words, 0) == 0);
    CHECK(same_state(f, g));

    run(f, 29, 35, ya);
    run(g, 29, 35, yb);
    CHECK(memcmp(ya, yb, 35 * sizeof(float)) == 0);
    CHECK(same_state(f, g));

    /* a clone is its own object: the original moves on, the clone of a clone stays */
    fxo_t* h = fxo_clone(g);
    run(f, 64, 7, ya);
    CHECK(!same_state(f, g) && same_state(g, h));
    int cur[4] = { 4, 9, 17, 2 }, got[4];
    fxo_set_cursors(h, cur);
    fxo_cursors(h, got);
    CHECK(memcmp(cur, got, sizeof cur) == 0);
    fxo_cursors(g, got);
    CHECK(memcmp(cur, got, sizeof cur) != 0);
    run(h, 64, 7, yb);

    /* a clone taken before the xTRAM exists (a program that never runs) */
    fxo_t* e = fxo_create(1);
    fxo_t* e2 = fxo_clone(e);
    CHECK(fxo_set_tram(e2, 1, 10, words, 5) == 5);
    CHECK(fxo_tram(e, 1, back, 16) == 16 && back[11] == 0.0f);
    fxo_destroy(e); fxo_destroy(e2);

    fxo_destroy(f); fxo_destroy(g); fxo_destroy(h);
    if (failures) return 1;
    puts("state_check ok");
    return 0;
}

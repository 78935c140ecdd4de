// test_scout_tables.cpp — build_scout_tables (csrc/hrx_defs.cpp: the tables of the chunked launch's scout) as a program of its own, built with
// -fsanitize=address,undefined by tests/test_plan_golden_cpu.py.  Three small def sets; the expectation is read off the narrow table, entry by entry:
//   - for every def, every row in [0, S + 2) and every byte, following the class LUT and then the u16 row address of the compact image lands on the row the
//     narrow table's entry for that (row, byte) names, and on row S + 1 for an undefined one
//   - qabs bit s is set exactly where every byte of the def's alphabet (the bytes some real state has a transition for) keeps real state s where it is
//   - a def of more than 127 byte classes yields no compact image
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../halo2_regex_amd/csrc/hrx_defs.cpp"

using namespace hrx;

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            ++failures;                                               \
        }                                                             \
    } while (0)

struct DefText { std::string allstr; std::vector<std::string> substrs; };

static DefsSet make_set(const std::vector<DefText> &defs) {
    DefsSet s;
    for (const DefText &t : defs) {
        RegexDefs rd;
        if (parse_allstr_text(t.allstr.data(), t.allstr.size(), rd.allstr)) { std::printf("allstr text does not parse\n"); ++failures; }
        for (const std::string &sub : t.substrs) {
            SubstrRegexDef sd;
            if (parse_substr_text(sub.data(), sub.size(), sd)) { std::printf("substr text does not parse\n"); ++failures; }
            rd.substrs.push_back(sd);
        }
        s.defs.push_back(rd);
    }
    std::string err;
    if (finalize_defs(s, err)) { std::printf("finalize: %s\n", err.c_str()); ++failures; }
    return s;
}

// "first\naccepted\nlargest\n" + "cur next byte" lines
static std::string allstr_of(unsigned largest, const std::vector<std::vector<unsigned>> &edges) {
    std::string t = "0\n" + std::to_string(largest) + "\n" + std::to_string(largest) + "\n";
    for (const auto &e : edges) t += std::to_string(e[0]) + " " + std::to_string(e[1]) + " " + std::to_string(e[2]) + "\n";
    return t;
}

// the narrow table's word on (row r of def d, byte c): the def-relative row it names, S + 1 where the entry is undefined
static uint32_t narrow_next(const DefsSet &s, uint32_t d, uint32_t r, uint32_t c, bool *defined = nullptr) {
    const DefConsts &k = s.consts[d];
    const uint32_t S = (uint32_t)s.defs[d].allstr.largest_state_val + 1, e = s.table_image[((size_t)k.row_base + r) * 256 + c];
    if (defined) *defined = e < k.dead_entry;
    return e < k.dead_entry ? (e >> kNextShift) - k.row_base : S + 1;
}

static void check_set(const char *name, const DefsSet &s, bool expect_compact, uint32_t expect_qabs_bits) {
    const ScoutTables t = build_scout_tables(s);
    EXPECT(t.cimage.empty() == !expect_compact);
    uint32_t qabs_bits = 0;
    for (uint32_t d = 0; d < s.defs.size(); ++d) {
        const uint32_t S = (uint32_t)s.defs[d].allstr.largest_state_val + 1;
        bool in_alphabet[256];
        for (uint32_t c = 0; c < 256; ++c) {
            in_alphabet[c] = false;
            for (uint32_t q = 0; q < S; ++q) { bool def; narrow_next(s, d, q, c, &def); in_alphabet[c] |= def; }
        }
        for (uint32_t q = 0; q < 256; ++q) {
            bool stays = q < S;
            for (uint32_t c = 0; c < 256 && stays; ++c) {
                bool def = false;
                const uint32_t nx = q < S ? narrow_next(s, d, q, c, &def) : 0;
                if (in_alphabet[c]) stays = def && nx == q;
            }
            const bool bit = (t.qabs[d][q >> 5] >> (q & 31)) & 1u;
            if (bit != stays) { std::printf("%s: def %u state %u: qabs %d, the table says %d\n", name, d, q, (int)bit, (int)stays); ++failures; }
            qabs_bits += bit;
        }
        if (t.cimage.empty()) continue;
        const uint32_t rowb = t.c_rowb[d], tab = t.c_tab[d];
        EXPECT(rowb >= 2 && rowb % 2 == 0 && rowb <= 254 && t.c_inv[d] == (65536u + rowb - 1u) / rowb);
        EXPECT((size_t)t.c_lut[d] + 256 <= t.cimage.size() && (size_t)tab + (size_t)(S + 2) * rowb <= t.cimage.size());
        for (uint32_t r = 0; r < S + 2; ++r)
            for (uint32_t c = 0; c < 256; ++c) {
                const uint32_t cls2 = t.cimage[t.c_lut[d] + c];
                uint16_t addr;
                std::memcpy(&addr, &t.cimage[(size_t)tab + (size_t)r * rowb + cls2], 2);
                const uint32_t want = narrow_next(s, d, r, c);
                if (cls2 >= rowb || addr < tab || (addr - tab) % rowb != 0 || (addr - tab) / rowb != want) {
                    std::printf("%s: def %u row %u byte %u: class %u, address %u, the narrow table names row %u\n", name, d, r, c, cls2 / 2, (unsigned)addr, want);
                    ++failures;
                    return;
                }
            }
    }
    EXPECT(qabs_bits == expect_qabs_bits);
}

int main() {
    // one def of three states: 2 is where every byte of the alphabet {a, b, c} stays (quasi-absorbing); 1 is not (b leaves it), 0 has no transition for c
    const DefText small{allstr_of(2, {{0, 1, 'a'}, {0, 0, 'b'}, {1, 1, 'a'}, {1, 2, 'b'}, {1, 1, 'c'}, {2, 2, 'a'}, {2, 2, 'b'}, {2, 2, 'c'}}), {"8\n0\n99\n1 \n2 \n1 2\n"}};
    check_set("one def", make_set({small}), true, 1);
    // two defs: a second one over other bytes, whose states 0 and 3 both stay (0 only because nothing leaves it: x and y loop there)
    const DefText other{allstr_of(3, {{0, 0, 'x'}, {0, 0, 'y'}, {1, 2, 'x'}, {1, 1, 'y'}, {2, 3, 'x'}, {2, 3, 'y'}, {3, 3, 'x'}, {3, 3, 'y'}}), {}};
    check_set("two defs", make_set({small, other}), true, 1 + 2);
    // one def of 140 states whose byte c < 139 leads from state 0 to state c + 1: 139 columns that differ, + the undefined one: more than 127 classes
    std::vector<std::vector<unsigned>> fan;
    for (unsigned c = 0; c < 139; ++c) fan.push_back({0, c + 1, c});
    check_set("many classes", make_set({DefText{allstr_of(139, fan), {}}}), false, 0);
    if (failures) return 1;
    std::printf("scout tables: ok\n");
    return 0;
}

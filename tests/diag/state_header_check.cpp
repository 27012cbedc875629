// Stand-alone check of csrc/qcart_state.hpp (no HIP, no GPU; tests/test_checkpoint_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a plain executable): encode a header, then feed the validator
//   - the intact blob (accepted),
//   - every truncation of it, each in a heap buffer of exactly that many bytes, so a read past the end is a
//     sanitizer report,
//   - one corruption per header word and per field part (name, type, pad, value), a flipped magic, a newer and a
//     zero format version, another kind, a padded buffer,
// and expect a refusal with a non-empty text for each. Exit status 0 and "ok" on stdout when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../deepreinforcementlearningcontrolofquantumcartpoles_amd/csrc/qcart_state.hpp"

namespace st = qcart::state;

static int failures = 0;

static void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::printf("FAIL: %s\n", what.c_str());
        ++failures;
    }
}

// validate a copy of blob[0 : n) held in a heap buffer of exactly n bytes
static std::string run(const std::vector<unsigned char>& blob, size_t n, const st::Header& mine) {
    unsigned char* buf = (unsigned char*)std::malloc(n ? n : 1);
    if (n) std::memcpy(buf, blob.data(), n);
    st::Header out;
    const std::string r = st::validate(buf, n, mine, &out);
    std::free(buf);
    return r;
}

int main() {
    const uint64_t payload = 40;
    st::Header h = st::make(st::kLearner);
    st::put_i(h, "data_length", 5);
    st::put_i(h, "hidden2", 256);
    st::put_i(h, "batch_size", 128);
    st::put_f(h, "gamma", 0.998);
    st::put_u(h, "seed", 0xfedcba9876543210ull);
    st::put_f(h, "a_name_of_23_characters", -0.0);   // the longest name that fits
    h.payload_bytes = payload;
    std::vector<unsigned char> blob(sizeof(h) + payload, 0xab);
    std::memcpy(blob.data(), &h, sizeof(h));

    expect(run(blob, blob.size(), h).empty(), "the intact blob is accepted: " + run(blob, blob.size(), h));
    st::Header out;
    expect(st::validate(nullptr, blob.size(), h, &out).size() > 0, "a null buffer is refused");

    // every truncation, down to the bare header and to nothing
    for (size_t n = 0; n < blob.size(); ++n) {
        const std::string r = run(blob, n, h);
        expect(!r.empty(), "truncation to " + std::to_string(n) + " bytes is refused");
        expect(r.find("truncated") != std::string::npos, "truncation to " + std::to_string(n) + " says so: " + r);
    }
    {   // one byte too many
        std::vector<unsigned char> b = blob;
        b.push_back(0);
        expect(!run(b, b.size(), h).empty(), "a padded buffer is refused");
    }

    // single corruptions of the header
    auto corrupt = [&](const char* what, const char* expect_word, auto edit) {
        st::Header c = h;
        edit(c);
        std::vector<unsigned char> b = blob;
        std::memcpy(b.data(), &c, sizeof(c));
        const std::string r = run(b, b.size(), h);
        expect(!r.empty(), std::string(what) + " is refused");
        expect(r.find(expect_word) != std::string::npos, std::string(what) + " names '" + expect_word + "': " + r);
    };
    corrupt("a flipped magic", "magic", [](st::Header& c) { c.magic ^= 1u; });
    corrupt("a fully flipped magic", "magic", [](st::Header& c) { c.magic = ~c.magic; });
    corrupt("a newer format", "format", [](st::Header& c) { c.format = st::kFormat + 1; });
    corrupt("format 0", "format", [](st::Header& c) { c.format = 0; });
    corrupt("another kind", "kind", [](st::Header& c) { c.kind = st::kMlearner; });
    corrupt("an unknown kind", "kind", [](st::Header& c) { c.kind = 77; });
    corrupt("fewer fields", "n_fields", [](st::Header& c) { c.n_fields -= 1; });
    corrupt("more fields", "n_fields", [](st::Header& c) { c.n_fields += 1; });
    corrupt("a huge field count", "n_fields", [](st::Header& c) { c.n_fields = 0xffffffffu; });
    corrupt("a shorter payload length", "truncated or padded", [](st::Header& c) { c.payload_bytes -= 1; });
    corrupt("a longer payload length", "truncated or padded", [](st::Header& c) { c.payload_bytes += 1; });
    corrupt("a huge payload length", "truncated or padded", [](st::Header& c) { c.payload_bytes = ~0ull; });
    corrupt("a set reserved word", "reserved", [](st::Header& c) { c.reserved = 1; });
    for (uint32_t i = 0; i < h.n_fields; ++i) {
        const std::string name = h.f[i].name;
        corrupt(("field " + name + ": value").c_str(), name.c_str(), [i](st::Header& c) { c.f[i].bits ^= 1ull << 40; });
        corrupt(("field " + name + ": name").c_str(), "names", [i](st::Header& c) { c.f[i].name[0] ^= 0x20; });
        corrupt(("field " + name + ": name without a terminator").c_str(), "names",
                [i](st::Header& c) { std::memset(c.f[i].name, 'x', st::kNameLen); });
        corrupt(("field " + name + ": type").c_str(), "type", [i](st::Header& c) { c.f[i].type += 1; });
        corrupt(("field " + name + ": pad").c_str(), "names", [i](st::Header& c) { c.f[i].pad = 1; });
    }
    corrupt("an entry past n_fields", "not empty", [&](st::Header& c) { c.f[h.n_fields].bits = 1; });
    corrupt("the last entry past n_fields", "not empty", [](st::Header& c) { c.f[st::kMaxFields - 1].name[0] = 'z'; });

    // a value mismatch names the field and both values
    {
        st::Header mine = h;
        mine.f[1].bits = 512;
        const std::string r = run(blob, blob.size(), mine);
        expect(r.find("hidden2") != std::string::npos && r.find("256") != std::string::npos &&
                   r.find("512") != std::string::npos,
               "a differing field is named with both values: " + r);
    }
    // more fields than the header holds are dropped by put(), never written past the array
    {
        st::Header full = st::make(st::kReplay);
        for (int i = 0; i < st::kMaxFields + 5; ++i) st::put_i(full, "f", i);
        expect(full.n_fields == (uint32_t)st::kMaxFields, "put() stops at kMaxFields");
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

// qcart_state.hpp — the header of a handle's exported state (qc_<kind>_state_export / _import, include/qcart.h):
// encode, print and validate. Host only, no HIP include: a blob is a fixed-size Header followed by the payload the
// handle's translation unit writes. The header names what the blob was made for as a list of (name, value) fields:
// the handle's create-time params and the geometry derived from them. An import compares the list with the
// receiving handle's own, field by field, and refuses on the first difference, naming it and both values.
// Internal: not part of the C ABI.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace qcart {
namespace state {

constexpr uint32_t kMagic = 0x54534351u;   // "QCST", little endian
constexpr uint32_t kFormat = 1;            // blob format version; a blob with a newer one is refused
constexpr int kMaxFields = 24;
constexpr int kNameLen = 24;
enum Kind : uint32_t { kActor = 1, kMactor = 2, kReplay = 3, kLearner = 4, kMlearner = 5, kSched = 6, kMonitor = 7 };
enum Type : uint32_t { kI64 = 0, kU64 = 1, kF64 = 2 };

struct Field {
    char name[kNameLen];   // NUL padded
    uint32_t type;         // Type
    uint32_t pad;
    uint64_t bits;         // the value's bit pattern (doubles compare bitwise)
};
struct Header {
    uint32_t magic, format, kind, n_fields;
    uint64_t payload_bytes;
    uint64_t reserved;
    Field f[kMaxFields];
};
static_assert(sizeof(Field) == 40 && sizeof(Header) == 32 + 40 * kMaxFields, "blob header layout");

inline const char* kind_name(uint32_t k) {
    switch (k) {
        case kActor: return "qc_actor";
        case kMactor: return "qc_mactor";
        case kReplay: return "qc_replay";
        case kLearner: return "qc_learner";
        case kMlearner: return "qc_mlearner";
        case kSched: return "qc_sched";
        case kMonitor: return "qc_monitor";
        default: return "unknown";
    }
}

inline Header make(uint32_t kind) {
    Header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = kMagic;
    h.format = kFormat;
    h.kind = kind;
    return h;
}

inline void put(Header& h, const char* name, uint32_t type, uint64_t bits) {
    if (h.n_fields >= (uint32_t)kMaxFields) return;
    Field& f = h.f[h.n_fields++];
    std::strncpy(f.name, name, kNameLen - 1);
    f.type = type;
    f.bits = bits;
}
inline void put_i(Header& h, const char* name, int64_t v) { put(h, name, kI64, (uint64_t)v); }
inline void put_u(Header& h, const char* name, uint64_t v) { put(h, name, kU64, v); }
inline void put_f(Header& h, const char* name, double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof(b));
    put(h, name, kF64, b);
}

inline std::string show(uint32_t type, uint64_t bits) {
    char buf[48];
    if (type == kF64) {
        double v;
        std::memcpy(&v, &bits, sizeof(v));
        std::snprintf(buf, sizeof(buf), "%.17g", v);
    } else if (type == kI64) {
        std::snprintf(buf, sizeof(buf), "%" PRId64, (int64_t)bits);
    } else {
        std::snprintf(buf, sizeof(buf), "%" PRIu64, bits);
    }
    return buf;
}

// Is `src` [n bytes] a complete blob for a handle whose own header is `mine`? Empty: yes, and *out holds the
// blob's header. Otherwise the refusal's text. Reads no byte at or past src + n; payload_bytes of `mine` is not
// compared (a payload whose length depends on its content is checked by the handle).
inline std::string validate(const void* src, uint64_t n, const Header& mine, Header* out) {
    const std::string who = std::string(kind_name(mine.kind)) + "_state_import: ";
    if (!src) return who + "null buffer";
    if (n < sizeof(Header))
        return who + "buffer truncated: " + std::to_string(n) + " bytes, the header alone has " +
               std::to_string(sizeof(Header));
    Header h;
    std::memcpy(&h, src, sizeof(h));
    if (h.magic != kMagic) return who + "magic: blob " + std::to_string(h.magic) + ", expected " + std::to_string(kMagic);
    if (h.format < 1 || h.format > kFormat)
        return who + "format: blob " + std::to_string(h.format) + ", this library reads up to " + std::to_string(kFormat);
    if (h.kind != mine.kind)
        return who + "kind: blob " + std::to_string(h.kind) + " (" + kind_name(h.kind) + "), handle " +
               std::to_string(mine.kind) + " (" + kind_name(mine.kind) + ")";
    if (h.n_fields != mine.n_fields)
        return who + "n_fields: blob " + std::to_string(h.n_fields) + ", handle " + std::to_string(mine.n_fields);
    if (h.reserved != 0) return who + "reserved: blob " + std::to_string(h.reserved) + ", expected 0";
    if (h.payload_bytes != n - sizeof(Header))
        return who + "buffer truncated or padded: " + std::to_string(n) + " bytes, the blob states " +
               std::to_string(sizeof(Header)) + " + " + std::to_string(h.payload_bytes);
    for (uint32_t i = 0; i < mine.n_fields; ++i) {
        const Field &a = h.f[i], &b = mine.f[i];
        if (std::memcmp(a.name, b.name, kNameLen) != 0 || a.type != b.type || a.pad != 0) {
            char nm[kNameLen + 1] = {0};
            std::memcpy(nm, a.name, kNameLen);
            return who + "field " + std::to_string(i) + ": blob names '" + nm + "' (type " + std::to_string(a.type) +
                   "), handle '" + b.name + "' (type " + std::to_string(b.type) + ")";
        }
        if (a.bits != b.bits)
            return who + b.name + ": blob " + show(a.type, a.bits) + ", handle " + show(b.type, b.bits);
    }
    for (int i = (int)mine.n_fields; i < kMaxFields; ++i) {
        static const Field zero = {};
        if (std::memcmp(&h.f[i], &zero, sizeof(Field)) != 0)
            return who + "field " + std::to_string(i) + ": not empty past n_fields";
    }
    if (out) *out = h;
    return std::string();
}

// a cursor over the payload: append on export, read on import (the caller has checked the length)
struct Cursor {
    unsigned char* p;
    explicit Cursor(void* base) : p((unsigned char*)base + sizeof(Header)) {}
    unsigned char* take(uint64_t bytes) {
        unsigned char* at = p;
        p += bytes;
        return at;
    }
};

}  // namespace state
}  // namespace qcart

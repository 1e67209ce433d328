// lab_guard_check.cpp — checks the host half of the lab stage harness (frankensearch_amd/csrc/lab_guard.hpp) on host buffers: the guard
// bands and bodies of collect_out, the guard rows behind a slab, the padded bitmap.  A plain program: tests/test_lab_guard_contract.py
// builds it with the address and undefined-behaviour sanitizers and runs it; it prints the first failed check and returns 1.
#include "lab_guard.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace lab = fsgpu::lab;
using Bytes = std::vector<unsigned char>;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

namespace {

// what the device would hold for `o`: both bands of the guard byte, the body as given (exactly o.total() bytes, so that a read or a
// write one byte outside is the sanitizer's)
Bytes image(const lab::Out& o, const Bytes& body) {
    Bytes h(o.total(), (unsigned char)lab::kGuardByte);
    std::memcpy(h.data() + o.band, body.data(), o.bytes);
    return h;
}

Bytes arbitrary(size_t n, unsigned seed) {
    Bytes b(n);
    for (size_t i = 0; i < n; ++i) b[i] = (unsigned char)((i * 131 + seed * 29 + (i >> 8)) & 0xff);
    return b;
}

// a byte-sized output of `bytes`: intact bands are no hit and the body arrives exactly; a flip at either end of either band is a hit
void check_byte_output(size_t bytes) {
    Bytes body = arbitrary(bytes, (unsigned)bytes);
    body[0] = (unsigned char)lab::kGuardByte;   // a body may hold the guard byte itself
    Bytes host(bytes, 0);
    lab::Out o;
    o.band = lab::kBand, o.bytes = bytes, o.host = host.data();
    CHECK(o.total() == bytes + 2 * 4096);
    const Bytes h = image(o, body);
    CHECK(!lab::collect_out(o, h.data()));
    CHECK(host == body);
    const size_t flips[4] = {0, o.band - 1, o.band + bytes, o.total() - 1};
    for (size_t at : flips) {
        Bytes bad = h;
        bad[at] ^= 0x01;
        std::fill(host.begin(), host.end(), 0);
        CHECK(lab::collect_out(o, bad.data()));
        CHECK(host == body);   // the body still arrives: the caller sees what the kernel wrote
    }
    // the last byte of the body and the first of it belong to the body, not to a band
    Bytes edge = h;
    edge[o.band] ^= 0xff, edge[o.band + bytes - 1] ^= 0xff;
    CHECK(!lab::collect_out(o, edge.data()));
}

// a row-shaped output as LabStage::out makes it: bands of 64 rows of its own width
void check_row_output() {
    const size_t rows = 3, row = 7 * 4;
    lab::Out o;
    Bytes host(rows * row, 0);
    o.band = 64 * row, o.bytes = rows * row, o.row = row, o.host = host.data();
    const Bytes body = arbitrary(o.bytes, 5);
    Bytes h = image(o, body);
    CHECK(!lab::collect_out(o, h.data()) && host == body);
    h[o.band + o.bytes] = 0;
    CHECK(lab::collect_out(o, h.data()));
    // widen: the caller converts, nothing is copied here, the bands are still judged
    lab::Out w = o;
    w.widen = true;
    std::fill(host.begin(), host.end(), 0x11);
    h = image(w, body);
    CHECK(!lab::collect_out(w, h.data()) && host == Bytes(host.size(), 0x11));
    h[w.band - 1] = 0;
    CHECK(lab::collect_out(w, h.data()));
}

// untouched: the whole body must still be guard bytes; nothing goes to a host
void check_untouched() {
    lab::Out o;
    o.band = 64 * 5, o.bytes = 9 * 5, o.untouched = true;
    const Bytes clean(o.bytes, (unsigned char)lab::kGuardByte);
    Bytes h = image(o, clean);
    CHECK(!lab::collect_out(o, h.data()));
    for (size_t at : {(size_t)0, o.bytes / 2, o.bytes - 1}) {
        Bytes bad = h;
        bad[o.band + at] = 0;
        CHECK(lab::collect_out(o, bad.data()));
    }
}

// slab_rows = m of 32: rows < m of every slab go to [slabs][m][row]; rows m..31 of every slab must keep the guard byte
void check_slab_rows(size_t m) {
    const size_t slabs = 4, row = 6 * 4;
    lab::Out o;
    Bytes host(slabs * m * row, 0);
    o.band = 64 * row, o.bytes = slabs * 32 * row, o.row = row, o.slab_rows = m, o.host = host.data();
    Bytes body(o.bytes, (unsigned char)lab::kGuardByte), want;
    for (size_t sl = 0; sl < slabs; ++sl) {
        const Bytes part = arbitrary(m * row, (unsigned)(sl + 1));
        std::memcpy(body.data() + sl * 32 * row, part.data(), part.size());
        want.insert(want.end(), part.begin(), part.end());
    }
    const Bytes h = image(o, body);
    CHECK(!lab::collect_out(o, h.data()));
    CHECK(host == want);
    for (size_t sl = 0; sl < slabs; ++sl) {
        // the first byte of row m and the last byte of row 31, in every slab (the last slab's row 31 ends where the band begins)
        for (size_t at : {sl * 32 * row + m * row, sl * 32 * row + 32 * row - 1}) {
            Bytes bad = h;
            bad[o.band + at] ^= 0x80;
            CHECK(lab::collect_out(o, bad.data()));
        }
        // the last byte of row m - 1 is the kernel's to write
        Bytes fine = h;
        fine[o.band + sl * 32 * row + m * row - 1] ^= 0x80;
        CHECK(!lab::collect_out(o, fine.data()));
    }
}

void check_guard_tails() {
    const size_t body = 48, pitch = 16, tail = 3 * pitch;
    const Bytes src = arbitrary(body, 9);
    const Bytes f16 = lab::with_guard_tail(src.data(), body, tail, lab::Tail::kF16NaN);
    const Bytes f32 = lab::with_guard_tail(src.data(), body, tail, lab::Tail::kF32NaN);
    const Bytes i8 = lab::with_guard_tail(src.data(), body, tail, lab::Tail::kByte7f);
    for (const Bytes* h : {&f16, &f32, &i8}) {
        CHECK(h->size() == body + tail);
        CHECK(std::memcmp(h->data(), src.data(), body) == 0);
    }
    for (size_t i = 0; i < tail; i += 2) CHECK(f16[body + i] == 0x00 && f16[body + i + 1] == 0x7e);
    static const unsigned char quad[4] = {0x00, 0x00, 0xc0, 0x7f};
    for (size_t i = 0; i < tail; ++i) CHECK(f32[body + i] == quad[i & 3]);
    for (size_t i = 0; i < tail; ++i) CHECK(i8[body + i] == 0x7f);
    // one row of one byte: the smallest body
    const Bytes one = lab::with_guard_tail(src.data(), 1, 16, lab::Tail::kF32NaN);
    CHECK(one.size() == 17 && one[0] == src[0] && one[1] == 0x00 && one[3] == 0xc0 && one[16] == 0x7f);
}

void check_bitmaps() {
    const size_t nrows[3] = {1, 64, 65}, words[3] = {1, 1, 2};
    for (int c = 0; c < 3; ++c) {
        CHECK(lab::bitmap_words(nrows[c]) == words[c]);
        std::vector<uint64_t> src(words[c]);   // exactly the words the caller owns: a read past them is the sanitizer's
        for (size_t i = 0; i < src.size(); ++i) src[i] = ~0ull - i;
        const std::vector<uint64_t> w = lab::padded_bitmap(src.data(), src.size());
        CHECK(w.size() == words[c] + 2);
        for (size_t i = 0; i < src.size(); ++i) CHECK(w[i] == src[i]);
        CHECK(w[words[c]] == 0 && w[words[c] + 1] == 0);
    }
    CHECK(lab::bitmap_words(0) == 0 && lab::bitmap_words(128) == 2 && lab::bitmap_words(129) == 3);
}

}  // namespace

int main() {
    CHECK(lab::kGuardByte == 0xA5 && lab::kBand == 4096);
    for (size_t bytes : {(size_t)1, (size_t)100, (size_t)4096, (size_t)12345}) check_byte_output(bytes);   // 100, 12345: no multiple of 16
    check_row_output();
    check_untouched();
    check_slab_rows(1);
    check_slab_rows(31);
    check_guard_tails();
    check_bitmaps();
    std::printf("lab_guard_check: ok\n");
    return 0;
}

// sphx_carve.h - the layout of a device buffer that holds several arrays, stated once (host code only, no HIP: it
// compiles in a plain C++17 program, tests/host/carve_check.cpp).
//
// A layout is an ordered list of pieces.  take(p, count, align) appends `count` elements behind the pieces so far, at the
// end of the previous piece rounded up to `align` bytes (default: the element's own alignment, where the offset is the
// running sum), and remembers the pointer variable p.  From that one list come the bytes to allocate - bytes() - and,
// once the buffer stands, every pointer - bind(base).  sphx_carve_into (sphx_internal.h) does both around sphx_ensure.
//   take(p, n, 16)   a piece on a 16-byte boundary: what sphx_excl_scan_int's 16-byte accesses need of its blocks
//   pad(16)          the end rounded up, so that the last such block is whole too
//   slack(bytes)     room behind the last piece that no pointer names
// A piece of count 0 takes no room and moves no later piece; its pointer is its rounded offset, inside bytes().
// No heap: room for MAX_PIECES pieces (32 in a Carve), and one more makes the layout overflowed() - an error at
// sphx_carve_into, no overrun.
#pragma once
#include <stddef.h>

template <int CAP> class CarveN {
public:
    enum { MAX_PIECES = CAP };
    template <class T> void take(T*& p, size_t count, size_t align = alignof(T)) {
        if (n_ == MAX_PIECES) { over_ = true; return; }
        const size_t off = (end_ + align - 1) / align * align;
        piece_[n_++] = Piece{&p, off, [](void* var, char* at) { *static_cast<T**>(var) = reinterpret_cast<T*>(at); }};
        if (count > 0) end_ = off + count * sizeof(T);
        if (top_ < off) top_ = off;
        if (top_ < end_) top_ = end_;
    }
    void pad(size_t align) { end_ = (end_ + align - 1) / align * align; if (top_ < end_) top_ = end_; }
    void slack(size_t bytes) { slack_ += bytes; }
    size_t bytes() const { return top_ + slack_; }
    bool overflowed() const { return over_; }
    int pieces() const { return n_; }
    size_t offset(int i) const { return piece_[i].off; }
    void bind(void* base) const {
        for (int i = 0; i < n_; ++i) piece_[i].set(piece_[i].var, static_cast<char*>(base) + piece_[i].off);
    }

private:
    struct Piece { void* var; size_t off; void (*set)(void* var, char* at); };
    Piece piece_[MAX_PIECES];
    int n_ = 0;
    bool over_ = false;
    size_t end_ = 0, top_ = 0, slack_ = 0;
};
typedef CarveN<32> Carve;               // (the radiative phase's 34 arrays take a CarveN<40>)

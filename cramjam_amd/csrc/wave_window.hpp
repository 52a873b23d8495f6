// wave_window.hpp — the one way to open the 512-byte register window (InWindow) over a stream of any alignment.  A template over the
// window's type and written against its documented members alone (base, iend, anchor), so that the same text serves cj_common.hpp's
// InWindow on the device and every host stand-in of it (tests/hostsim) that the *_wave.hpp headers are compiled over.
#pragma once

namespace cj {

// the window over the n bytes at `in`: base = the dword boundary at or below in, iend and the first anchor relative to it; returns the
// position of in[0] relative to base (0..3)
template <class Window>
__device__ __forceinline__ uint32_t window_open(Window& w, const uint8_t* in, uint32_t n) {
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(in) & 3u);
    w.base = in - mis;
    w.iend = mis + n;
    w.anchor(mis);
    return mis;
}

}  // namespace cj

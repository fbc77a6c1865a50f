// Constants of the half-band stages that host code needs too (the bank planner, chan_plan.cpp): no HIP headers.
// A constexpr function is host and device code alike under hipcc.
#pragma once
#include <stdint.h>

namespace sdrx {

constexpr int HIST = 32;           // history entries kept in front of every polyphase array

constexpr uint32_t HBM_BIAS2 = 0x00800080u;      // XORed into every packed odd-arm dword an MFMA stage reads (hb_mfma.hpp)

constexpr uint32_t pk16(int lo, int hi)
{
    return (uint32_t)(uint16_t)(int16_t)lo | ((uint32_t)(uint16_t)(int16_t)hi << 16);
}

} // namespace sdrx

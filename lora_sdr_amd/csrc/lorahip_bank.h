// What the two polyphase banks (lorahip_pfb.hip, the channeliser; lorahip_psb.hip, the synthesis bank) have in common, stated once:
// the bin counts M they accept -- a power of two 8..1024 or 5 * 2^a, a = 0..6 -- with the limits and the refusals, the twiddle table
// of the transform (lorahip_pfbfft.h, lorahip_pfbfft5.h) and where it leaves a bin, the tile rule, and the step from the M of an
// object to the M a kernel is compiled for.
#pragma once
#include "lorahip_frontend.h"
#include "lorahip_pfbfft5.h"
#include <cmath>
#include <type_traits>
#include <utility>

namespace lorahip {

constexpr int BANK_LOGM_MIN = 3, BANK_LOGM_MAX = 10;    // M = 2^logM
constexpr int BANK_A_MAX = 6;                           // M = 5 * 2^a, a = 0 .. 6
//! every M a bank is compiled for
using BankCounts = std::integer_sequence<int, 8, 16, 32, 64, 128, 256, 512, 1024, 5, 10, 20, 40, 80, 160, 320>;

constexpr bool bankIsPow2(const int M) { return (M & (M - 1)) == 0; }
constexpr int bankLog2(const int n) { return n <= 1 ? 0 : 1 + bankLog2(n >> 1); }
//! the radix-2 part of M: M itself, or M / 5
constexpr int bankPow2Part(const int M) { return bankIsPow2(M) ? M : M / 5; }
//! entries of the twiddle table: the N / 2 roots of the radix-2 part N; 5 * 2^a: then the M roots of the radix-5 stage
constexpr int bankTwiddles(const int M) { return bankIsPow2(M) ? M / 2 : M / 10 + M; }
//! log2 of the tile: T = the largest power of two with T M <= 4096, 2^minLogT at least and 256 at most
constexpr int bankLogT(const int M, const int minLogT)
{
    const int logT = bankLog2(4096 / M);
    return logT < minLogT ? minLogT : (logT > 8 ? 8 : logT);
}

//! where bin (or residue) b = 5 k + r, 0 <= b < M, stands in a row after the transform: r N + bitrev(k); a power of two: bitrev(b)
inline int bankPlace(const int M, const int b)
{
    const int N = bankPow2Part(M), logN = bankLog2(N), fifth = bankIsPow2(M) ? 1 : 5;
    const unsigned k = unsigned(b / fifth);
    unsigned rev = 0;
    for (int bit = 0; bit < logN; bit++) rev |= ((k >> bit) & 1u) << (logN - 1 - bit);
    return (b % fifth) * N + int(rev);
}

//! the same in a kernel (M = 5: no radix-2 stage, k = 0, and no shift by 32)
template <int M>
__device__ __forceinline__ int bankPlaceDev(const int b)
{
    constexpr int N = bankPow2Part(M), LOGN = bankLog2(N), FIFTH = bankIsPow2(M) ? 1 : 5;
    const int k = int(unsigned(b) / unsigned(FIFTH)), r = b - FIFTH * k;
    int at = r * N;
    if constexpr (LOGN > 0) at += int(__brev(unsigned(k)) >> (32 - LOGN));
    return at;
}

//! a signed bin modulo M, in [0, M)
inline int bankBin(const int M, const int32_t b) { return int(((long long)b % M + M) % M); }

//! the table of bankTwiddles(M) entries, computed in double: exp(-+2 pi i k / N), k < N / 2, N the radix-2 part of M; 5 * 2^a: then
//! exp(-+2 pi i n / M), n < M. The forward transform takes the minus sign, the inverse the plus sign
inline std::vector<float2> bankTwiddleTable(const int M, const bool inverse)
{
    std::vector<float2> tw;
    tw.reserve(size_t(bankTwiddles(M)));
    const auto root = [&tw, inverse](const int k, const int P)
    {
        const double ang = 2.0 * M_PI * double(k) / double(P);
        tw.push_back(make_float2(float(std::cos(ang)), float(inverse ? std::sin(ang) : -std::sin(ang))));
    };
    const int N = bankPow2Part(M);
    for (int k = 0; k < N / 2; k++) root(k, N);
    if (!bankIsPow2(M))
        for (int n = 0; n < M; n++) root(n, M);
    return tw;
}

//! LORAHIP_OK when the shape is one a bank handles; otherwise LORAHIP_E_INVALID, and lorahip_last_error says why: "<who>: ...", who =
//! the bank, rateWord = what it calls its rate change (decim, interp)
inline int bankCheck(const std::string &who, const std::string &rateWord, const bool radix5, const size_t nBins, const size_t rate,
                     const size_t nTaps, const size_t nSel)
{
    const size_t n = nBins / 5;
    const bool badBins = radix5 ? nBins % 5 || n == 0 || n > (size_t(1) << BANK_A_MAX) || (n & (n - 1))
                                : nBins < (size_t(1) << BANK_LOGM_MIN) || nBins > (size_t(1) << BANK_LOGM_MAX) || (nBins & (nBins - 1));
    std::string why;
    if (badBins && radix5) why = "n_bins of the radix-5 bank must be 5 * 2^a, a = 0..6 (5, 10, 20, 40, 80, 160 or 320)";
    else if (badBins) why = "n_bins must be a power of two in 8..1024";
    else if (rate == 0 || rate > 4096) why = rateWord + " must be 1..4096";
    else if (nTaps == 0 || nTaps > (size_t(1) << 16)) why = "n_taps must be 1..65536";
    else if (nSel == 0 || nSel > size_t(65535) * 8) why = "n_sel must be 1..524280";
    if (why.empty()) return LORAHIP_OK;
    setLastError(who + ": " + why);
    return LORAHIP_E_INVALID;
}

//! f(std::integral_constant<int, M>()) for the M of a bank object, one of Ms (BankCounts): from the value at run time to the
//! template argument of the kernels
template <int... Ms, class F>
hipError_t bankDispatch(const int M, std::integer_sequence<int, Ms...>, F &&f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((M == Ms && ((e = f(std::integral_constant<int, Ms>())), true)) || ...);
    return e;
}

} // namespace lorahip

// The transmit frame walk of the modulator kernels (lora_sdr_amd/csrc/lorahip_framewalk.h) on its own: a plain C++ program over that
// header and the standard library, no HIP, no GPU. tests/test_framewalk_cpu.py builds it with the library's floating-point flags
// (-ffp-contract=off -fno-fast-math) and compares what it writes, bit for bit, with tests/modulator_def.py::mod_phases_def.
//
//   framewalk_check OUT sf sync S  count sym[0] .. sym[S-1]  count sym[0] .. sym[S-1]  ...
//
// walks one frame per (count, S symbols) group exactly as modFrames walks a row of lorahip_mod_frames_var with max_nsyms = S -- every
// chirp of the body, 15 + S of them -- and writes to OUT, frame by frame, the float32 phase of every body sample (0 where the sample
// belongs to a zero chirp) and then one byte per body sample: 1 where it is a chirp sample, 0 where not. Phases only: cos / sin of them
// are the device's own (polar() is not compiled here).
#include "lorahip_framewalk.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 5) { std::fprintf(stderr, "framewalk_check: OUT sf sync S (count sym*S)...\n"); return 2; }
    const int sf = std::atoi(argv[2]), sync = std::atoi(argv[3]), S = std::atoi(argv[4]);
    if (sf < 6 || sf > 12 || S < 1 || (argc - 5) % (S + 1) != 0) { std::fprintf(stderr, "framewalk_check: bad arguments\n"); return 2; }
    const int N = 1 << sf, frames = (argc - 5) / (S + 1);
    std::FILE *out = std::fopen(argv[1], "wb");
    if (out == nullptr) { std::perror(argv[1]); return 2; }
    for (int fr = 0; fr < frames; fr++)
    {
        char **a = argv + 5 + fr * (S + 1);
        std::vector<unsigned short> syms(S);
        for (int k = 0; k < S; k++) syms[k] = (unsigned short)std::atoi(a[1 + k]);
        std::vector<float> phase;
        std::vector<unsigned char> live;
        int nsyms = std::atoi(a[0]);
        if (nsyms > S) nsyms = -1;                                         // more than the row holds: silent, as modFrames has it
        lorahip::FrameWalk w(N);
        for (int c = 0; c < 15 + S; c++)
        {
            w.chirp(c, sync, syms.data(), nsyms);
            for (int i = 0; i < w.NN; i++)
            {
                phase.push_back(w.zero ? 0.0f : w.next());
                live.push_back(w.zero ? 0 : 1);
            }
            if (!w.zero) w.endChirp();
        }
        if (std::fwrite(phase.data(), sizeof(float), phase.size(), out) != phase.size() || std::fwrite(live.data(), 1, live.size(), out) != live.size())
        {
            std::perror(argv[1]);
            return 2;
        }
    }
    if (std::fclose(out) != 0) { std::perror(argv[1]); return 2; }
    std::printf("framewalk_check: %d frames\n", frames);
    return 0;
}

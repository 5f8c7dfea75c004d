// pwm_host_machine.cpp — the path rr_pwm_decoder replaces, on one host core: the sequential machine of
// rustradio_amd/csrc/pwm_host.hpp over a file of f32 power samples (tools/pwm_probe.py builds and runs it).
// usage: pwm_host_machine power.f32 short long tol frame_gap reset_gap frame_bits min_repeats delimiter repeats
// prints one line per repeat: "<frames> <milliseconds>"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rustradio_amd/csrc/pwm_host.hpp"

int main(int argc, char** argv) {
    if (argc != 11) { std::printf("usage: %s power.f32 short long tol frame_gap reset_gap frame_bits min_repeats delimiter repeats\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / sizeof(float);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> x(n);
    if (n && std::fread(x.data(), sizeof(float), n, f) != n) { std::printf("short read\n"); return 2; }
    std::fclose(f);
    auto arg = [&](int i) { return (size_t)std::strtoull(argv[i], nullptr, 10); };
    const rr::PwmCfg c = rr::pwm_cfg(0.5f, 0.25f, arg(2), arg(3), arg(4), arg(5), arg(6), arg(7), 4096, 256, arg(8), arg(9) ? RR_PWM_GAP_DELIMITER : 0);
    for (size_t r = 0; r < arg(10); r++) {
        rr::PwmMachine m(c);
        std::vector<rr::PwmHostFrame> out;
        const auto t0 = std::chrono::steady_clock::now();
        m.push(x.data(), n, out);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%zu %.4f\n", out.size(), ms);
    }
    return 0;
}

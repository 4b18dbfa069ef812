// copy_games.cpp — bboard::BatchEnvironment::CopyGames / CopyGamesDevice (include/pom_bboard.hpp) from C++: games drawn and
// played on the device, a fan-out and an in-place resample by host indices, a masked resample by device indices; every copied
// game's State equals its source's byte for byte, the others are untouched.
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "pom_bboard.hpp"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("REQUIRE failed line %d: %s\n", __LINE__, #c);   \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static std::vector<bboard::State> all(bboard::BatchEnvironment& env)
{
    const bboard::State* s = env.GetStates();
    return std::vector<bboard::State>(s, s + env.Size());
}
static bool same(const bboard::State& a, const bboard::State& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    const int64_t n = 200;
    bboard::BatchEnvironment env(n, 0, POM_RESET_AT_START, 800);
    env.MakeGame(uint64_t(5));
    env.StepSimpleAgents(9, 25);

    // fan-out: games 40..89 become copies of games 0..4
    std::vector<bboard::State> before = all(env);
    std::vector<int64_t> src(50);
    for (int i = 0; i < 50; i++) src[size_t(i)] = i % 5;
    env.CopyGames(src.data(), 40, 50);
    for (int64_t e = 0; e < n; e++) {
        const bboard::State& want = (e >= 40 && e < 90) ? before[size_t(src[size_t(e - 40)])] : before[size_t(e)];
        REQUIRE(same(env.GetState(e), want));
    }
    int differ = 0;
    for (int i = 0; i < 5; i++) differ += !same(before[size_t(i)], before[size_t(i + 1)]);
    REQUIRE(differ > 0);

    // in place, with repeats, over the whole batch
    before = all(env);
    std::vector<int64_t> perm(static_cast<size_t>(n));
    for (int64_t e = 0; e < n; e++) perm[size_t(e)] = (e * 37 + 11) % 97;
    env.CopyGames(perm.data(), 0, n);
    for (int64_t e = 0; e < n; e++) REQUIRE(same(env.GetState(e), before[size_t(perm[size_t(e)])]));

    // device indices: odd entries -1 (left alone)
    env.StepSimpleAgents(9, 5);
    before = all(env);
    for (int64_t e = 0; e < n; e++) perm[size_t(e)] = (e & 1) ? -1 : n - 1 - e;
    int64_t* dev = nullptr;
    REQUIRE(hipMalloc((void**)&dev, size_t(n) * sizeof(int64_t)) == hipSuccess);
    REQUIRE(hipMemcpy(dev, perm.data(), size_t(n) * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess);
    env.CopyGamesDevice(dev, 0, n);
    const std::vector<bboard::State> after = all(env);
    for (int64_t e = 0; e < n; e++) REQUIRE(same(after[size_t(e)], perm[size_t(e)] < 0 ? before[size_t(e)] : before[size_t(perm[size_t(e)])]));
    REQUIRE(hipFree(dev) == hipSuccess);

    // bad indices are refused and change nothing
    bool threw = false;
    try {
        std::vector<int64_t> bad{0, n};
        env.CopyGames(bad.data(), 0, 2);
    } catch (const std::exception&) {
        threw = true;
    }
    REQUIRE(threw);
    const std::vector<bboard::State> unchanged = all(env);
    for (int64_t e = 0; e < n; e++) REQUIRE(same(unchanged[size_t(e)], after[size_t(e)]));
    std::printf("copy games ok\n");
    return 0;
}

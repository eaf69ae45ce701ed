// format_emulation.cpp — csrc/gple_format.hip compiled for the host (tests/test_format_host.py): every thread of a workgroup is a host thread,
// __syncthreads a barrier, __shfl_up an exchange through memory, workgroups run one after another.  It checks what needs no GPU: the items'
// layout, both scans, the offsets, the staging at the destination's alignment and that no byte outside the text is written — against
// snprintf("%g"), for both write-pass variants.  It says nothing about the device's own execution (tests/test_gpu_format.py does).
#define __HIP_PLATFORM_AMD__
#include <hip/hip_runtime.h>
#include <algorithm>
#include <barrier>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <thread>
#include <vector>
using std::max;
using std::min;
struct Idx { unsigned x = 0, y = 0, z = 0; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<>* g_bar = nullptr;
static unsigned g_slots[1024];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline unsigned __shfl_up(unsigned v, int d)
{
	const unsigned t = threadIdx.x;
	g_slots[t] = v;
	g_bar->arrive_and_wait();
	const unsigned r = static_cast<int>(t & 63) >= d ? g_slots[t - d] : v;
	g_bar->arrive_and_wait();
	return r;
}
static void emu_launch(unsigned grid, unsigned block, const std::function<void()>& body)
{
	std::barrier<> bar(block);
	g_bar = &bar;
	std::vector<std::thread> ts;
	for (unsigned t = 0; t < block; ++t)
		ts.emplace_back([&, t] {
			for (unsigned b = 0; b < grid; ++b)
			{
				threadIdx.x = t;
				blockIdx.x = b;
				body();
				bar.arrive_and_wait(); // the next workgroup reuses the static "LDS"
			}
		});
	for (auto& th : ts) th.join();
}
#undef __shared__
#define __shared__ static
#undef __launch_bounds__
#define __launch_bounds__(x)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) emu_launch((grid).x, (block).x, [&] { k(__VA_ARGS__); })
#include "../../gaussian_process_liouville_equation_amd/csrc/gple_format.hip"

int main()
{
	std::vector<uint64_t> table(gple_g6::TABLE_WORDS);
	gple_g6::build_table(table.data());
	std::mt19937_64 rng(5);
	int bad = 0;
	struct Shape { size_t per_line, lines, lpb; };
	for (Shape s : {Shape{1, 5, 0}, {7, 3, 1}, {257, 3, 0}, {1024, 1, 1}, {1025, 1, 0}, {3, 700, 7}})
		for (int join = 0; join < 2; ++join)
			{
				const int slots = join ^ (s.per_line == 1025); // both write-pass variants, spread over the set
				const size_t count = s.per_line * s.lines;
				std::vector<double> v(count);
				for (double& x : v)
				{
					const uint64_t b = rng();
					if (b & 1) std::memcpy(&x, &b, 8);
					else x = static_cast<double>(static_cast<int64_t>(b >> 40)) * 1e-3 - 8000.0;
					if ((b & 0xff0) == 0) x = -1.23457e-308;
				}
				std::string want;
				char buf[64];
				for (size_t i = 0; i < count; ++i)
				{
					if (!(join && i % s.per_line == 0)) want += ' ';
					std::snprintf(buf, sizeof buf, "%g", v[i]);
					if (!std::strcmp(buf, "-nan")) std::strcpy(buf, "nan");
					want += buf;
					if ((i + 1) % s.per_line == 0)
					{
						want += '\n';
						if (s.lpb && ((i + 1) / s.per_line) % s.lpb == 0) want += '\n';
					}
				}
				const size_t bound = 14 * count + s.lines + (s.lpb ? s.lines / s.lpb : 0);
				std::vector<unsigned char> work(gple::format_work_bytes(count, slots) + 16), text(bound + 64, 0xAB);
				void* w = work.data() + (16 - reinterpret_cast<uintptr_t>(work.data()) % 16) % 16;
				for (int off : {join ? 0 : 5}) // destination alignment
				{
					std::fill(text.begin(), text.end(), 0xAB);
					const unsigned long long* len = nullptr;
					(void)gple::launch_format(nullptr, v.data(), count, s.per_line, s.lpb, join, reinterpret_cast<const unsigned long long*>(table.data()), w, slots,
						reinterpret_cast<char*>(text.data()) + 16 + off, &len);
					const bool ok = *len == want.size() && *len <= bound && !std::memcmp(text.data() + 16 + off, want.data(), want.size()) &&
						text[16 + off - 1] == 0xAB && text[16 + off + want.size()] == 0xAB;
					if (!ok) ++bad, std::printf("BAD shape %zu x %zu / %zu join %d slots %d off %d: len %llu want %zu\n", s.per_line, s.lines, s.lpb, join, slots, off, *len, want.size());
				}
			}
	std::printf("emulation done, %d bad\n", bad);
	return bad != 0;
}

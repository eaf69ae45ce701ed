// gple_capi_sharded.hip — C-ABI entry points of include/gple.h: the grid-sharded and dealt predicts (RCCL all-gather) and the batched point-predict.
#include <algorithm>
#include <cmath>
#include <dlfcn.h>
#include <string>

#include "gple_capi.h"

extern "C"
{
	// ---- grid-sharded predict: slice -> predict -> ncclAllGather -> unpack ------------------------------------------------------
	int gple_shard_bounds(size_t M, int rank, int world, size_t* lo, size_t* hi, size_t* per)
	{
		if (world <= 0 || rank < 0 || rank >= world) return GPLE_ERR_BAD_ARG;
		const size_t p = M ? (M + static_cast<size_t>(world) - 1) / static_cast<size_t>(world) : 0; // parallel.shard_bounds
		const size_t l = std::min(M, static_cast<size_t>(rank) * p), h = std::min(M, l + p);
		if (lo) *lo = l;
		if (hi) *hi = h;
		if (per) *per = p;
		return GPLE_OK;
	}
	namespace
	{
		// RCCL's C entry point, resolved lazily: from the process image when the caller links librccl (their ncclComm_t then
		// belongs to that very library), else from librccl.so.1.  No RCCL header or link dependency in this library.
		using allgather_fn = int (*)(const void*, void*, size_t, int, void*, hipStream_t);
		std::atomic<allgather_fn> allgather_override{nullptr};
		allgather_fn resolve_allgather()
		{
			if (allgather_fn o = allgather_override.load()) return o;
			static allgather_fn fn = [] {
				void* sym = nullptr;
				if (const char* named = getenv("GPLE_RCCL_LIBRARY")) // the caller names the library its ncclComm_t comes from: nothing else is tried
				{
					if (void* h = dlopen(named, RTLD_NOW | RTLD_GLOBAL)) sym = dlsym(h, "ncclAllGather");
					return reinterpret_cast<allgather_fn>(sym);
				}
				sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
				if (!sym)
					for (const char* name : {"librccl.so.1", "librccl.so"})
						if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))
							if ((sym = dlsym(h, "ncclAllGather"))) break;
				return reinterpret_cast<allgather_fn>(sym);
			}();
			return fn;
		}
		// Block-cyclic deal of the test points.  Contiguous slices would balance the full contraction just as well, but with far-row
		// pruning (the default) the live blocks of a phase-space grid sit in one corner of it and a contiguous slice holds anything
		// between all and none of them.  Plain deal: 128-point block b belongs to rank b % world (local block b / world).  Weighted deal
		// (plans that give the ranks unequal shares of an element): out of every cycle of S = sum(w) consecutive blocks rank
		// r takes the w[r] blocks cum[r] .. cum[r] + w[r] - 1; the plain deal is w = 1 for everyone.
		constexpr size_t SHARD_BLOCK = 128;
		constexpr int DEAL_MAX_WORLD = 64;
		struct Deal
		{
			int world, S;
			int cum[DEAL_MAX_WORLD + 1];
			__host__ __device__ int weight(int r) const { return cum[r + 1] - cum[r]; }
			__host__ __device__ int owner(size_t b) const
			{
				const int p = static_cast<int>(b % S);
				int r = 0;
				while (cum[r + 1] <= p) ++r;
				return r;
			}
			// block `lb` of rank r's share -> block of the grid
			__host__ __device__ size_t global_block(int r, size_t lb) const { return (lb / weight(r)) * S + cum[r] + lb % weight(r); }
			// block b of the grid (owned by r) -> block of r's share
			__host__ __device__ size_t local_block(int r, size_t b) const { return (b / S) * weight(r) + (b % S - cum[r]); }
			size_t blocks_of(int r, size_t nblocks) const
			{
				const size_t rem = nblocks % S, w = static_cast<size_t>(weight(r)), c = static_cast<size_t>(cum[r]);
				return (nblocks / S) * w + (rem > c ? std::min(rem - c, w) : 0);
			}
		};
		bool make_deal(int world, const int* weights, Deal& d)
		{
			if (world < 1 || world > DEAL_MAX_WORLD) return false;
			d.world = world, d.cum[0] = 0;
			for (int r = 0; r < world; ++r)
			{
				const int w = weights ? weights[r] : 1;
				if (w < 0 || w > (1 << 20)) return false;
				d.cum[r + 1] = d.cum[r] + w;
			}
			d.S = d.cum[world];
			return d.S > 0;
		}
		__global__ void __launch_bounds__(256) shard_points_kernel(const double* __restrict__ Xs, size_t M, int rank, Deal deal, size_t n_local,
			double* __restrict__ out)
		{
			const size_t j = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
			if (j >= n_local) return;
			const size_t i = deal.global_block(rank, j / SHARD_BLOCK) * SHARD_BLOCK + j % SHARD_BLOCK;
			out[2 * j] = Xs[2 * i], out[2 * j + 1] = Xs[2 * i + 1];
		}
		// gathered[r][...] (world blocks of (2 ow + 1) * per doubles: mean | var | cut of rank r's points) -> full-length outputs
		__global__ void __launch_bounds__(256) unshard_kernel(const double* __restrict__ g, size_t per, int ow, size_t M, Deal deal, double* __restrict__ mean,
			double* __restrict__ var, double* __restrict__ cut)
		{
			const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
			if (i >= M) return;
			const size_t b = i / SHARD_BLOCK;
			const int r = deal.owner(b);
			const size_t q = deal.local_block(r, b) * SHARD_BLOCK + i % SHARD_BLOCK;
			const double* __restrict__ blk = g + r * (2 * ow + 1) * per;
			for (int k = 0; k < ow; ++k)
			{
				if (mean) mean[ow * i + k] = blk[ow * q + k];
				if (cut) cut[ow * i + k] = blk[(ow + 1) * per + ow * q + k];
			}
			if (var) var[i] = blk[ow * per + q];
		}
		// rank's share under a deal: its number of points and the padded share length every rank allocates
		void deal_counts(const Deal& d, size_t M, int rank, size_t& n_local, size_t& per)
		{
			const size_t nblocks = (M + SHARD_BLOCK - 1) / SHARD_BLOCK;
			size_t most = 0;
			for (int r = 0; r < d.world; ++r) most = std::max(most, d.blocks_of(r, nblocks));
			per = most * SHARD_BLOCK;
			n_local = d.blocks_of(rank, nblocks) * SHARD_BLOCK;
			if (nblocks && d.owner(nblocks - 1) == rank) n_local -= nblocks * SHARD_BLOCK - M; // owner of the short block: it is the last of its share
		}
	} // namespace
	// Rehearsal transport for ONE rank of a world that is not there (bench.py --emulate-rank r/P on a one-GPU box): ncclAllGather's signature;
	// `comm` is not a communicator but the number 1 + rank + 256 * world.  This rank's block lands in its slot, the other ranks' slots are
	// zero-filled (roughly the HBM writes a real gather makes; the fabric's share of the time is what the rehearsal cannot show).
	int gple_debug_solo_allgather(const void* sendbuff, void* recvbuff, size_t sendcount, int datatype, void* comm, void* hip_stream)
	{
		hipStream_t stream = static_cast<hipStream_t>(hip_stream);
		const size_t code = reinterpret_cast<size_t>(comm);
		if (datatype != 8 || code < 257) return 4;
		const size_t world = (code - 1) / 256, rank = (code - 1) % 256;
		if (rank >= world) return 4;
		char* dst = static_cast<char*>(recvbuff);
		const size_t blk = sendcount * sizeof(double);
		if (rank > 0 && hipMemsetAsync(dst, 0, rank * blk, stream) != hipSuccess) return 1;
		if (rank + 1 < world && hipMemsetAsync(dst + (rank + 1) * blk, 0, (world - rank - 1) * blk, stream) != hipSuccess) return 1;
		return hipMemcpyAsync(dst + rank * blk, sendbuff, blk, hipMemcpyDeviceToDevice, stream) == hipSuccess ? 0 : 1;
	}
	int gple_set_allgather_function(void* fn)
	{
		allgather_override.store(reinterpret_cast<allgather_fn>(fn));
		return GPLE_OK;
	}
	static int predict_sharded(gple_ctx* ctx, const FitCommon* f, bool is_complex, const double* Xs, size_t M, unsigned flags, int rank, int world, const int* weights,
		void* comm, double* prediction, double* variance, double* cutoff_prediction)
	{
		if (world < 1 || rank < 0 || rank >= world) return GPLE_ERR_BAD_ARG;
		if (world > 1 && !comm) return GPLE_ERR_BAD_ARG;
		Deal deal;
		if (!make_deal(world, weights, deal)) return GPLE_ERR_BAD_ARG;
		if (!f && deal.weight(rank) > 0) return GPLE_ERR_BAD_ARG; // only a rank without a share may come without the fit
		if (M == 0) return GPLE_OK;
		const bool dev = flags & GPLE_IO_DEVICE;
		if (!comm) return predict_common(ctx, f, Xs, M, flags & (GPLE_IO_DEVICE | GPLE_PREDICT_FULL), nullptr, prediction, variance, cutoff_prediction, nullptr);
		const allgather_fn allgather = resolve_allgather();
		if (!allgather)
		{
			std::lock_guard<std::mutex> lk(ctx->mu);
			const char* de = dlerror(); // one call: dlerror() clears the state it returns
			ctx->last_error = std::string("ncclAllGather not found: ") + (de ? de : "librccl is not loadable");
			return GPLE_ERR_COLLECTIVE;
		}
		// this rank's points: its blocks of every cycle (the last block of the grid may be short)
		size_t n_local = 0, per = 0;
		deal_counts(deal, M, rank, n_local, per);
		const size_t ow = is_complex ? 2 : 1, blk = (2 * ow + 1) * per;
		hipStream_t st = ctx->stream;
		// the points go through device buffers whatever the caller's pointers are: the collective runs on device memory
		Scratch local(ctx), gathered(ctx), xs(ctx);
		Staged xs_all(ctx, dev), om(ctx, dev), ov(ctx, dev), oc(ctx, dev);
		{
			GPLE_CALL(ctx);
			GPLE_HIP(ctx, local.get(blk));
			GPLE_HIP(ctx, gathered.get(blk * world));
			GPLE_HIP(ctx, hipMemsetAsync(local.p, 0, blk * 8, st)); // the padded tail of the ranks with fewer points
			GPLE_HIP(ctx, xs_all.in(Xs, 2 * M));
			if (n_local)
			{
				GPLE_HIP(ctx, xs.get(2 * n_local));
				hipLaunchKernelGGL(shard_points_kernel, dim3(static_cast<unsigned>((n_local + 255) / 256)), dim3(256), 0, st, xs_all.p, M, rank, deal, n_local, xs.p);
				GPLE_HIP(ctx, hipGetLastError());
			}
		}
		// A rank whose own predict fails still enters the collective (with whatever its buffer holds: the other ranks get their
		// result, this one reports its error afterwards) -- returning here would leave every other rank waiting in ncclAllGather.
		// Only a failure to allocate the collective's own buffers above returns early; the caller then has to abort the communicator.
		int rc_local = GPLE_OK;
		std::string err_local;
		if (n_local)
		{
			rc_local = predict_common(ctx, f, xs.p, n_local, GPLE_IO_DEVICE | (flags & GPLE_PREDICT_FULL), nullptr, local.p, local.p + ow * per,
				local.p + (ow + 1) * per, nullptr);
			if (rc_local != GPLE_OK)
			{
				std::lock_guard<std::mutex> l2(ctx->mu);
				err_local = ctx->last_error;
			}
		}
		GPLE_CALL(ctx);
		const int rc = allgather(local.p, gathered.p, blk, /* ncclDouble */ 8, comm, st);
		if (rc != 0)
		{
			std::lock_guard<std::mutex> l2(ctx->mu);
			ctx->last_error = "ncclAllGather returned " + std::to_string(rc);
			return GPLE_ERR_COLLECTIVE;
		}
		if (rc_local != GPLE_OK)
		{
			GPLE_HIP(ctx, hipStreamSynchronize(st)); // the scratch buffers go back to the pool when this returns
			std::lock_guard<std::mutex> l2(ctx->mu);
			ctx->last_error = err_local;
			return rc_local;
		}
		GPLE_HIP(ctx, om.out(prediction, ow * M));
		GPLE_HIP(ctx, ov.out(variance, M));
		GPLE_HIP(ctx, oc.out(cutoff_prediction, ow * M));
		hipLaunchKernelGGL(unshard_kernel, dim3(static_cast<unsigned>((M + 255) / 256)), dim3(256), 0, st, gathered.p, per, static_cast<int>(ow), M, deal, om.p, ov.p,
			oc.p);
		GPLE_HIP(ctx, hipGetLastError());
		for (Staged* o : {&om, &ov, &oc}) GPLE_HIP(ctx, o->back());
		if (!dev)
		{
			GPLE_HIP(ctx, hipStreamSynchronize(st));
			timer_collect(ctx);
		}
		return GPLE_OK;
	}
	int gple_real_predict_sharded(gple_ctx* ctx, const gple_real_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
		void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction)
	{
		if (!ctx || !fit || (M && !Xs)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		return predict_sharded(ctx, fit, false, Xs, M, flags, rank, world, nullptr, nccl_comm, prediction, variance, cutoff_prediction);
	}
	int gple_complex_predict_sharded(gple_ctx* ctx, const gple_complex_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
		void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction)
	{
		if (!ctx || !fit || (M && !Xs)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		return predict_sharded(ctx, fit, true, Xs, M, flags, rank, world, nullptr, nccl_comm, prediction, variance, cutoff_prediction);
	}
	int gple_real_predict_dealt(gple_ctx* ctx, const gple_real_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
		const int* weights, void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction)
	{
		if (!ctx || (M && !Xs)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		return predict_sharded(ctx, fit, false, Xs, M, flags, rank, world, weights, nccl_comm, prediction, variance, cutoff_prediction);
	}
	int gple_complex_predict_dealt(gple_ctx* ctx, const gple_complex_fit* fit, const double* Xs, size_t M, unsigned flags, int rank, int world,
		const int* weights, void* nccl_comm, double* prediction, double* variance, double* cutoff_prediction)
	{
		if (!ctx || (M && !Xs)) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		return predict_sharded(ctx, fit, true, Xs, M, flags, rank, world, weights, nccl_comm, prediction, variance, cutoff_prediction);
	}
	int gple_deal_share(size_t M, int rank, int world, const int* weights, size_t* n_local, size_t* per, size_t* indices)
	{
		Deal deal;
		if (rank < 0 || rank >= world || !make_deal(world, weights, deal)) return GPLE_ERR_BAD_ARG;
		size_t nl = 0, p = 0;
		deal_counts(deal, M, rank, nl, p);
		if (n_local) *n_local = nl;
		if (per) *per = p;
		if (indices)
			for (size_t j = 0; j < nl; ++j) indices[j] = deal.global_block(rank, j / SHARD_BLOCK) * SHARD_BLOCK + j % SHARD_BLOCK;
		return GPLE_OK;
	}

	// ---- batched point-predict (N1): gather -> one predict per element -> scatter ------------------------------------
	int gple_predict_batch(gple_ctx* ctx, const gple_element* elements, size_t n_elements, const double* points, const int* element_of_request,
		size_t n_req, double* out)
	{
		if (!ctx || (n_elements && !elements) || (n_req && (!points || !element_of_request || !out))) return GPLE_ERR_BAD_ARG;
		GPLE_OPEN(ctx);
		std::vector<std::vector<size_t>> by_element(n_elements);
		for (size_t r = 0; r < n_req; ++r)
		{
			const int e = element_of_request[r];
			if (e < 0 || static_cast<size_t>(e) >= n_elements) return GPLE_ERR_BAD_ARG;
			by_element[e].push_back(r);
		}
		std::vector<double> pts, cut;
		int status = GPLE_OK; // an element's GPLE_ERR_TIMEOUT (earlier work on its fit came out NaN; its results here are good) ends the batch
		for (size_t e = 0; e < n_elements; ++e)
		{
			const std::vector<size_t>& req = by_element[e];
			if (req.empty()) continue;
			const gple_element& el = elements[e];
			if (el.real && el.cplx) return GPLE_ERR_BAD_ARG;
			if (!el.real && !el.cplx) // element without a kernel: 0 (main.cpp:86-88, 97-99)
			{
				for (size_t r : req) out[2 * r] = out[2 * r + 1] = 0.0;
				continue;
			}
			const size_t m = req.size();
			pts.resize(2 * m);
			for (size_t q = 0; q < m; ++q) pts[2 * q] = points[2 * req[q]], pts[2 * q + 1] = points[2 * req[q] + 1];
			const FitCommon* f = el.real ? static_cast<const FitCommon*>(el.real) : static_cast<const FitCommon*>(el.cplx);
			cut.resize(el.real ? m : 2 * m);
			const int st = predict_common(ctx, f, pts.data(), m, GPLE_PREDICT_FULL, nullptr, nullptr, nullptr, cut.data(), nullptr);
			if (!own_outputs_written(st, f)) return st;
			if (st != GPLE_OK) status = st;
			for (size_t q = 0; q < m; ++q)
				out[2 * req[q]] = el.real ? cut[q] : cut[2 * q], out[2 * req[q] + 1] = el.real ? 0.0 : cut[2 * q + 1];
		}
		return status;
	}
}

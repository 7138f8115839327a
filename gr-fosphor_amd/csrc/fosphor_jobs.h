/*
 * fosphor_jobs.h -- the job-table substrate of the passes over burst IQ (fosphor_extract.hip, fosphor_resample.hip,
 * fosphor_measure.hip, fosphor_demod.hip, fosphor_correlate.hip, fosphor_psd.hip, fosphor_symbols.hip, fosphor_carrier.hip,
 * fosphor_decide.hip, fosphor_decode.hip, fosphor_soft.hip, fosphor_rs.hip); DESIGN.md, "the job-table substrate"
 *
 * A pass checks the caller's jobs on the host, sorts them into at most two forms, and uploads per form its device jobs and a prefix
 * of their work-group counts; a work-group finds its job by a bounded binary search of that prefix and its place in the job from
 * what is left.  A pass supplies its device job struct, the work-group size of each form and its kernels.  It gets from here:
 *   device  find_job(), and load_span(): a span of float32 IQ into an LDS image by 16-byte loads that read no byte outside the span;
 *   host    the refusals every pass shares, the packer of the table, and the tail of a call: upload, launch, check, count, drain.
 * The scratch buffers that hold the tables belong to the instance (fosphor_api.cpp); fosphor_pass.h names their slots and holds the
 * checked launch and the drain, which the passes over the plain buffers (fosphor_ring.h) end a call with as well.
 */
#ifndef FOSPHOR_JOBS_H
#define FOSPHOR_JOBS_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "fosphor_pass.h"					/* the scratch slots, the counters, launch and drain */

namespace job_table {

constexpr int kSearchSteps = 13;			/* 2^12 jobs: every pass asserts that its MAX_JOBS fits */
constexpr int kMaxJobs = 1 << (kSearchSteps - 1);
constexpr long long kMaxGroups = 0x7fffffffLL;		/* work-groups of one launch */

/* ---- device ---- */

/* the job of work-group g: the largest j with prefix[j] <= g.  A job without work-groups shares its prefix with the next and is
 * never the largest. */
__device__ __forceinline__ int find_job(const uint32_t *prefix, int n_jobs, uint32_t g)
{
	int lo = 0, hi = n_jobs;
	for (int step = 0; step < kSearchSteps && hi - lo > 1; step++) {
		const int mid = (lo + hi) >> 1;
		if (prefix[mid] <= g)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

/* y[0 .. count) for 16-byte loads: `head` (0 or 1) samples before the first 16-byte boundary, `pairs` pairs from it on, and the
 * single sample y[tail] behind the last pair if tail < count */
struct Span {
	int head, pairs, tail;
};

__device__ __forceinline__ Span split_span(const float2 *y, int count)
{
	Span s;
	s.head = min(count, (int)(((uintptr_t)y >> 3) & 1));
	s.pairs = (count - s.head) >> 1;
	s.tail = s.head + 2 * s.pairs;
	return s;
}

template <class S>
__device__ __forceinline__ S to_image(float re, float im)
{
	S v;
	v.x = re;
	v.y = im;
	return v;
}

/* Samples y[0 .. count) into the LDS image, by the kThreads lanes of a work-group of which this is lane t; count >= 1.
 * -> the image index of y[0] (0 or 1); y[m] lands at that index + m, at most at index count: a pair lands on a 16-byte boundary of a
 * float2 image too.  Reads y[0 .. count) and nothing else.  A float2 image takes a pair in one statement (routed through a helper by
 * value, the compiler spent 128 registers on it); any other element type is converted sample by sample. */
template <int kThreads, class S>
__device__ __forceinline__ int load_span(S *image, const float2 *y, int count, int t)
{
	const Span s = split_span(y, count);
	if (t == 0 && s.head) {
		if constexpr (std::is_same<S, float2>::value)
			image[1] = y[0];
		else
			image[1] = to_image<S>(y[0].x, y[0].y);
	}
	for (int g = t; g < s.pairs; g += kThreads) {
		if constexpr (std::is_same<S, float2>::value) {
			*reinterpret_cast<float4 *>(image + 2 * s.head + 2 * g) = *reinterpret_cast<const float4 *>(y + s.head + 2 * g);
		} else {
			const float4 q = *reinterpret_cast<const float4 *>(y + s.head + 2 * g);
			image[2 * s.head + 2 * g] = to_image<S>(q.x, q.y);
			image[2 * s.head + 2 * g + 1] = to_image<S>(q.z, q.w);
		}
	}
	if (t == kThreads - 1 && s.tail < count) {
		if constexpr (std::is_same<S, float2>::value)
			image[s.head + s.tail] = y[s.tail];
		else
			image[s.head + s.tail] = to_image<S>(y[s.tail].x, y[s.tail].y);
	}
	return s.head;
}

/* ---- host: what every pass refuses ---- */

inline bool count_ok(int n_jobs, int max_jobs) { return n_jobs >= 1 && n_jobs <= max_jobs; }

/* [offset, offset + n) inside [0, total): a job's samples inside the caller's, its outputs inside the capacity */
inline bool inside(int64_t offset, int64_t n, int64_t total)
{
	return offset >= 0 && n >= 0 && offset <= total && n <= total - offset;
}

/* the work-groups of n items at `per` a work-group */
inline long long groups_of(long long n, int per) { return (n + per - 1) / per; }

/* ... added to a form's running total, which has to stay a launch's grid */
inline bool add_groups(long long &total, long long n, int per)
{
	total += groups_of(n, per);
	return total <= kMaxGroups;
}

/* no two of the [first, second) ranges share an element; sorts them */
inline bool ranges_disjoint(std::vector<std::pair<int64_t, int64_t> > &ranges)
{
	std::sort(ranges.begin(), ranges.end());
	for (size_t i = 1; i < ranges.size(); i++)
		if (ranges[i].first < ranges[i - 1].second)
			return false;
	return true;
}

/* ---- host: the table ---- */

/* The table as it lies in the scratch buffer: the device jobs of form 0, those of form 1, the prefix of form 0, the prefix of form 1
 * and, where the pass has partial records, room for them from the next 8-byte boundary on.  A form or a prefix that a pass does not
 * have is empty.  `image` is what is uploaded, `bytes` what the buffer has to hold; the offsets are in bytes. */
struct Table {
	std::vector<uint8_t> image;
	size_t jobs_at[2], prefix_at[2], parts_at, bytes;
};

/* the layout alone, the image zeroed: for a pass that knows its counts beforehand and writes its jobs where they go */
inline Table lay_table(size_t job_bytes, const size_t (&n_form)[2], const size_t (&n_prefix)[2], size_t n_parts, size_t part_bytes)
{
	Table t;
	size_t at = 0;
	for (int f = 0; f < 2; f++) {
		t.jobs_at[f] = at;
		at += job_bytes * n_form[f];
	}
	for (int f = 0; f < 2; f++) {
		t.prefix_at[f] = at;
		at += sizeof(uint32_t) * n_prefix[f];
	}
	if (part_bytes)
		at = (at + 7) & ~(size_t)7;
	t.parts_at = at;
	t.bytes = at + part_bytes * n_parts;
	t.image.resize(at);
	return t;
}

template <class J>
Table pack_table(const std::vector<J> (&form)[2], const std::vector<uint32_t> (&prefix)[2], size_t n_parts, size_t part_bytes)
{
	const size_t n_form[2] = { form[0].size(), form[1].size() }, n_prefix[2] = { prefix[0].size(), prefix[1].size() };
	Table t = lay_table(sizeof(J), n_form, n_prefix, n_parts, part_bytes);
	for (int f = 0; f < 2; f++) {
		if (!form[f].empty())
			memcpy(t.image.data() + t.jobs_at[f], form[f].data(), sizeof(J) * form[f].size());
		if (!prefix[f].empty())
			memcpy(t.image.data() + t.prefix_at[f], prefix[f].data(), sizeof(uint32_t) * prefix[f].size());
	}
	return t;
}

/* ---- host: the tail of a call ---- */

/* The table into the pass's scratch buffer, on the instance's stream; the caller has called fosphor_amd_finish().  The image lives
 * on the host until drain(). */
inline int upload_table(struct fosphor *self, int which, const Table &t, uint8_t **d, hipStream_t *st)
{
	void *p;
	if (fosphor_amd_priv_scratch(self, which, t.bytes, &p))
		return -EIO;
	*st = (hipStream_t)fosphor_amd_stream(self);
	if (hipMemcpyAsync(p, t.image.data(), t.image.size(), hipMemcpyHostToDevice, *st) != hipSuccess)
		return -EIO;
	*d = static_cast<uint8_t *>(p);
	return 0;
}

/* the checked launch and the drain: fosphor_pass.h */
using pass::launch_ok;
using pass::launch;
using pass::drain;

} // namespace job_table

#endif

// pwn_players.cpp -- the players' step (pwn_players_step, pwn_players_step_device): a batch of cameras walked through the level
// in force by host/player.c's tick, on the device (player_step.hip).  The device form is one launch on the caller's stream; the
// host form stages its arrays like the blocking ray calls (pwn_calls.cpp) and ends with its stream drained.
#include <math.h>
#include <string.h>
#include "pwn_internal.h"

// What both forms refuse on their numbers alone (include/pwnhip.h)
static bool step_numbers_ok(int n, float tdiff, int ticks)
{
	return n >= 0 && n <= PWN_PLAYERS_MAX && ticks >= 1 && ticks <= PWN_TICKS_MAX && isfinite(tdiff);
}

// The launch of both forms, on stream s: behind the upload of the tables in force, from the walk table their copy refers to, and the
// copy guarded against the next upload into it.  No work-queue counters, no rotation, no stats.
static int step_launch(pwn_ctx *c, int n, const uint8_t *d_keys, float tdiff, int ticks, float *d_cams, float *d_gravity, int32_t *d_traversals, hipStream_t s)
{
	// (a level whose upload failed is sent again; tables that cannot be packed refuse the call before anything is launched)
	if(c->blob_dirty) { const int rc = pwn_i_pack_blob(c); if(rc != PWN_OK) return rc; }
	const int cur = c->blob_cur;
	const int rc = pwn_i_tables_uploaded(c, cur, s);
	if(rc != PWN_OK) return rc;
	// every workgroup copies the walk table into LDS first: never slower than reading it where it lies, 12-15 % faster over 64 ticks
	// (profiles/players/step.txt; PWN_PLAYERS_STAGE=0 of the environment is the other arm of that comparison)
	const int stage = c->dbg_players_stage >= 0 ? c->dbg_players_stage : 1;
	HIPCHK(c, pwn_launch_players_step(d_cams, d_gravity, d_traversals, d_keys, n, tdiff, ticks, c->d_walk[c->walk_of[cur]], stage, s));
	// The copy's guard is one event, and a record on s replaces the one before it.  Steps may come on any stream (include/pwnhip.h), so
	// where the last step that read this copy went out on another stream the upload stream is put behind THAT record first: every
	// later upload -- into this copy, or into a buffer this copy hands back -- then comes behind the steps of every stream.
	if(c->walk_in_use[cur] && c->walk_stream[cur] != s) HIPCHK(c, hipStreamWaitEvent(c->up_stream, c->ev_walk[cur], 0));
	HIPCHK(c, hipEventRecord(c->ev_walk[cur], s));
	c->walk_in_use[cur] = true; c->walk_stream[cur] = s;
	return PWN_OK;
}

extern "C" int pwn_players_step_device(pwn_ctx *c, int n, const void *d_keys, float tdiff, int ticks,
	void *d_cams, void *d_gravity, void *d_traversals, void *stream)
{
	GRP_REFUSE(c, "pwn_players_step_device");
	if(c == NULL || !step_numbers_ok(n, tdiff, ticks) || (n > 0 && (d_keys == NULL || d_cams == NULL || d_gravity == NULL))) return PWN_EINVAL;
	if((((uintptr_t)d_cams | (uintptr_t)d_gravity) & 15u) != 0 || ((uintptr_t)d_traversals & 3u) != 0) return PWN_EINVAL;
	{
		const uintptr_t N = (uintptr_t)n;
		const uintptr_t p[4] = { (uintptr_t)d_keys, (uintptr_t)d_cams, (uintptr_t)d_gravity, (uintptr_t)d_traversals }, b[4] = { N, 64 * N, 16 * N, 4 * N };
		for(int i = 0; i < 4; i++) for(int k = i + 1; k < 4; k++)
			if(p[i] != 0 && p[k] != 0 && p[i] < p[k] + b[k] && p[k] < p[i] + b[i]) return PWN_EINVAL;
	}
	const int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	return step_launch(c, n, (const uint8_t *)d_keys, tdiff, ticks, (float *)d_cams, (float *)d_gravity, (int32_t *)d_traversals, (hipStream_t)stream);
}

// The host form's staging for a call of n players: the cameras at 0 (64 B a player), the gravities at 64 n, the traversal counts at
// 80 n, the key bytes at 84 n -- 85 B a player, one copy up, one down (without the keys; without the counts where the caller has none)
extern "C" int pwn_players_step(pwn_ctx *c, int n, const uint8_t *keys, float tdiff, int ticks, float *cams, float *gravity, int32_t *traversals)
{
	GRP_REFUSE(c, "pwn_players_step");
	if(c == NULL || !step_numbers_ok(n, tdiff, ticks) || (n > 0 && (keys == NULL || cams == NULL || gravity == NULL))) return PWN_EINVAL;
	int rc = pwn_i_batch_refuse(c);
	if(rc != PWN_OK || n == 0) return rc;
	(void)hipSetDevice(c->device);
	hipStream_t s = c->stream;
	rc = pwn_i_wait_frames_in_flight(c, s);
	if(rc != PWN_OK) return rc;
	rc = pwn_i_staging_reserve(c, (size_t)n, 85, "pwn_players_step", &c->h_players, &c->d_players, &c->players_cap, PWN_PLAYERS_MAX, "players");
	if(rc != PWN_OK) return rc;
	const size_t N = (size_t)n;
	unsigned char *h = c->h_players, *d = c->d_players;
	memcpy(h, cams, 64 * N);
	memcpy(h + 64 * N, gravity, 16 * N);
	if(traversals != NULL) memcpy(h + 80 * N, traversals, 4 * N); else memset(h + 80 * N, 0, 4 * N);
	memcpy(h + 84 * N, keys, N);
	// (small batches by the upload kernel, as the ray calls: a DMA copy queues behind other copies of the device)
	if(85 * N <= 65536) HIPCHK(c, pwn_launch_upload(h, d, (85 * N + 15) & ~(size_t)15, s));
	else HIPCHK(c, hipMemcpyAsync(d, h, 85 * N, hipMemcpyHostToDevice, s));
	rc = step_launch(c, n, d + 84 * N, tdiff, ticks, (float *)d, (float *)(d + 64 * N), traversals != NULL ? (int32_t *)(d + 80 * N) : NULL, s);
	if(rc != PWN_OK) return rc;
	const size_t down = traversals != NULL ? 84 * N : 80 * N;
	HIPCHK(c, hipMemcpyAsync(h, d, down, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s));
	memcpy(cams, h, 64 * N);
	memcpy(gravity, h + 64 * N, 16 * N);
	if(traversals != NULL) memcpy(traversals, h + 80 * N, 4 * N);
	return PWN_OK;
}

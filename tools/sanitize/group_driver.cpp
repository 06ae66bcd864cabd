// The host logic of the row tiling and of the group (pwn_tiled.cpp, pwn_group.cpp and the host API's files they stand on) under ThreadSanitizer and
// AddressSanitizer + UBSan, on the CPU: fake HIP runtime, stand-in kernels (fake_kernels.cpp).  Every frame of a group of N
// members -- blocking calls, frames in flight delivered to the host, frames left on the devices -- must equal the frame of ONE
// context, bit for bit, with moving cuts, with a band of deep pixels that leaves the halo (repeat with whole strips), with
// depth that carries over, with a member that is late past the deadline (PWN_ETIMEDOUT, then recovery), and with
// processes over the shared-memory transport.  And after a call that went wrong (pwn_init_multi's `errors`, include/pwnhip.h): a
// refusal gives one context's code and leaves the group as it was (`refusals`), a real failure is reported per lost slot and
// mended (`lost`).  tools/sanitize/README.txt
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <sys/wait.h>
#include <vector>
#include "pwnhip.h"
#include "pwn_internal.h"       // (pwn_group_member, for the `lost` mode's members that disagree)

static const char *LEVEL =
	"###########\r\n#;;;;;;;;;#\r\n#;;*;;;;;;#\r\n#;;;;$$;;;#\r\n#;a;;;;;b;#\r\n#;;;;;;;;;#\r\n###########\r\n";
#define CK(call) do { int rc_ = (call); if(rc_ < 0) { fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, ctx ? pwn_last_error(ctx) : ""); exit(1); } } while(0)

static void cam_for(float cam[16], int f)
{
	memset(cam, 0, 64);
	cam[0] = cam[5] = cam[10] = cam[15] = 1.0f;
	cam[12] = 3.5f + 0.01f * (float)f; cam[13] = 0.5f; cam[14] = 2.5f;
}

static void spheres_for(std::vector<pwn_sphere> &s, int f)
{
	s.clear();
	for(int i = 0; i < 5 + f % 3; i++) { pwn_sphere q = { 0.2f, 0.3f, 2.0f + 0.3f * (float)i + 0.01f * (float)f, 0.4f, 2.0f + 0.2f * (float)i, 0.1f, 0.5f, 0.9f }; s.push_back(q); }
}

// frame f's sec: from frame 20 on a band of deep pixels (fake_kernels.cpp) whose taps leave the halo
static float sec_for(int f) { return f < 20 ? 0.25f * (float)f : 100.0f + 0.7f * (float)f; }

static int run_frames(pwn_ctx *ctx, int w, int h, int frames, std::vector<std::vector<uint32_t>> &out, std::vector<std::vector<float>> &zout, int mode)
{
	const size_t n = (size_t)w * h;
	std::vector<pwn_sphere> sph;
	float cam[16];
	if(mode == 0)
	{
		std::vector<uint32_t> sb(n); std::vector<float> zb(n);
		for(int f = 0; f < frames; f++)
		{
			spheres_for(sph, f); cam_for(cam, f);
			CK(pwn_upload_spheres(ctx, sph.data(), (int)sph.size()));
			CK(pwn_trace_screen_centred(ctx, cam, sec_for(f), sb.data(), zb.data()));
			out.push_back(sb); zout.push_back(zb);
		}
		return 0;
	}
	// frames in flight: mode 1 delivered to the host, mode 2 left on the device(s), mode 3 delivered with the upscaled surface (pitch wider than the rows)
	const int scale = 2, pitch = w * scale * 4 + 16;
	if(mode == 3) CK(pwn_frames_config(ctx, 3, PWN_FRAME_SBUF | PWN_FRAME_SURFACE, scale, pitch));
	else CK(pwn_frames_config(ctx, 3, mode == 1 ? (PWN_FRAME_SBUF | PWN_FRAME_ZBUF) : 0, 1, 0));
	std::vector<uint32_t> tmp(n);
	for(int f = 0; f < frames + 3; f++)
	{
		if(f >= 3)
		{
			pwn_frame fr;
			CK(pwn_wait_frame(ctx, f % 3, &fr));
			if(mode == 1) { out.push_back(std::vector<uint32_t>(fr.sbuf, fr.sbuf + n)); zout.push_back(std::vector<float>(fr.zbuf, fr.zbuf + n)); }
			else if(mode == 3)
			{
				// (screen.h:132,138-139: a source row takes w*scale + pitch*(scale-1) words of the surface)
				std::vector<uint32_t> both(fr.sbuf, fr.sbuf + n);
				const size_t rowadv = (size_t)w * scale + (size_t)(pitch / 4) * (scale - 1);
				both.insert(both.end(), fr.surface, fr.surface + rowadv * (size_t)h);
				out.push_back(both);
			}
			else { CK(pwn_read_plane(ctx, fr.d_sbuf, tmp.data(), n * 4)); out.push_back(tmp); }
		}
		if(f < frames)
		{
			spheres_for(sph, f); cam_for(cam, f);
			CK(pwn_upload_spheres(ctx, sph.data(), (int)sph.size()));
			CK(pwn_submit_frame(ctx, cam, sec_for(f), f % 3));
		}
	}
	CK(pwn_frames_config(ctx, 0, 0, 1, 0));
	return 0;
}

static int same(const std::vector<std::vector<uint32_t>> &a, const std::vector<std::vector<uint32_t>> &b, const char *what, int members)
{
	if(a.size() != b.size()) { fprintf(stderr, "%s, %d members: %zu frames against %zu\n", what, members, a.size(), b.size()); return 1; }
	for(size_t f = 0; f < a.size(); f++)
		if(a[f] != b[f])
		{
			size_t i = 0;
			while(a[f][i] == b[f][i]) i++;
			fprintf(stderr, "%s, %d members: frame %zu differs first at pixel %zu\n", what, members, f, i);
			return 1;
		}
	return 0;
}

static int group_runs(int w, int h)
{
	const int frames = 30;
	pwn_ctx *ctx = NULL;
	std::vector<std::vector<uint32_t>> ref[4]; std::vector<std::vector<float>> zref[4];
	for(int mode = 0; mode < 4; mode++)
	{
		CK(pwn_init(&ctx, 0, w, h));
		CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
		run_frames(ctx, w, h, frames, ref[mode], zref[mode], mode);
		pwn_destroy(ctx); ctx = NULL;
	}
	int bad = 0;
	for(int members = 2; members <= 5; members++)
		for(int mode = 0; mode < 4; mode++)
		{
			int devs[8];
			for(int i = 0; i < members; i++) devs[i] = (mode == 2) ? i : 0;       // (distinct ordinals too: the peer-copy branch of the transport)
			CK(pwn_init_multi(&ctx, devs, members, w, h));
			CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
			std::vector<std::vector<uint32_t>> got; std::vector<std::vector<float>> zgot;
			run_frames(ctx, w, h, frames, got, zgot, mode);
			bad |= same(ref[mode], got, mode == 0 ? "blocking" : mode == 1 ? "delivered" : mode == 2 ? "resident" : "surface", members);
			// (depth: a pixel the trace leaves alone keeps the previous call's value, or the value of the frame that had the slot before)
			if(mode < 2) for(size_t f = 0; f < zgot.size(); f++) if(memcmp(zgot[f].data(), zref[mode][f].data(), zgot[f].size() * 4) != 0) { fprintf(stderr, "%s, %d members: depth of frame %zu differs\n", mode == 0 ? "blocking" : "delivered", members, f); bad = 1; break; }
			pwn_group_info gi;
			CK(pwn_group_info_get(ctx, &gi));
			// (a bounded halo is in force to begin with where the shortest strip of the equal split holds it: the deep band then forces a repeat)
			const int per = ((h + members - 1) / members + 7) / 8 * 8, last = h - per * (members - 1), halo = (int)(0.002 * h * 24.0) + 2;
			const bool bounded = (last < per ? last : per) >= halo;
			if(gi.members != members || gi.transport != PWN_TRANSPORT_LOCAL || (bounded && gi.frames_redone == 0)) { fprintf(stderr, "%d members: info members %d transport %d redone %llu\n", members, gi.members, gi.transport, (unsigned long long)gi.frames_redone); bad = 1; }
			pwn_stats st;
			CK(pwn_get_stats(ctx, &st));
			pwn_destroy(ctx); ctx = NULL;
		}
	printf("group runs %dx%d: %s\n", w, h, bad ? "FAILED" : "every frame of 2..5 members equals the one-context frame (blocking, delivered, resident)");
	return bad;
}

// a member that is late past the deadline: PWN_ETIMEDOUT (or the failure it causes in the others), then the handle works again
static int late_member(void)
{
	const int w = 64, h = 96;
	pwn_ctx *ctx = NULL;
	int devs[3] = { 0, 0, 0 };
	setenv("PWN_DBG_GROUP_STALL", "1:3:900", 1);
	CK(pwn_init_multi(&ctx, devs, 3, w, h));
	unsetenv("PWN_DBG_GROUP_STALL");
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_tiled_set_timeouts(ctx, 5000, 200));
	std::vector<uint32_t> sb((size_t)w * h), first;
	float cam[16];
	cam_for(cam, 0);
	int errors = 0;
	for(int f = 0; f < 6; f++)
	{
		const int rc = pwn_trace_screen_centred(ctx, cam, 0.5f, sb.data(), NULL);
		if(rc != PWN_OK) { errors++; printf("late member: call %d -> %d (%s)\n", f + 1, rc, pwn_last_error(ctx)); continue; }
		if(first.empty()) first = sb;
		else if(first != sb) { fprintf(stderr, "late member: frame %d differs\n", f); return 1; }
	}
	pwn_destroy(ctx);
	if(errors != 1) { fprintf(stderr, "late member: %d calls failed, expected exactly the third\n", errors); return 1; }
	printf("late member: one call failed at the deadline, the others delivered the same frame\n");
	return 0;
}

// processes over the shared-memory transport (pwn_tiled_* as a process per GPU uses it)
static int shm_ranks(int world)
{
	const int w = 64, h = 160, frames = 12;
	unsigned char id[PWN_TILED_ID_BYTES];
	pwn_ctx *ctx = NULL;
	CK(pwn_tiled_unique_id(id, PWN_TRANSPORT_SHM));
	std::vector<pid_t> kids;
	int rank = 0;
	fflush(NULL);
	for(int r = 1; r < world; r++) { pid_t k = fork(); if(k == 0) { rank = r; kids.clear(); break; } kids.push_back(k); }
	CK(pwn_init(&ctx, 0, w, h));
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_tiled_set_timeouts(ctx, 20000, 20000));
	CK(pwn_tiled_init(ctx, rank, world, id, PWN_TRANSPORT_SHM, -1));
	std::vector<pwn_sphere> sph;
	float cam[16];
	unsigned long long sum = 0;
	for(int f = 0; f < frames + 2; f++)
	{
		if(f < frames) { spheres_for(sph, f); cam_for(cam, f); CK(pwn_upload_spheres(ctx, sph.data(), (int)sph.size())); CK(pwn_tiled_submit(ctx, cam, sec_for(f + 14))); }
		if(f >= 2)
		{
			pwn_tiled_frame tf;
			CK(pwn_tiled_wait(ctx, PWN_TILED_HOST, &tf));
			if(rank == 0) for(size_t i = 0; i < (size_t)w * h; i += 13) sum += tf.sbuf[i];
		}
	}
	pwn_tiled_shutdown(ctx);
	pwn_destroy(ctx);
	if(rank != 0) _exit(0);
	int bad = 0;
	for(pid_t k : kids) { int st = 0; if(waitpid(k, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) bad = 1; }
	printf("shm ranks %d: %s (checksum %llx)\n", world, bad ? "FAILED" : "done", sum);
	return bad;
}

// ---- refusals: a call that one context refuses, a group refuses with the same code, and goes on as one context goes on ---------
// A script is a list of steps; a step is a call of include/pwnhip.h and gives (return code, hash of every output the call filled).
// The same script runs on a one-context handle and on groups; the transcripts must be equal step by step.  Where the refusal is a
// group's own rule (no one-context counterpart) the one-context side of the step is the code the header states.
enum
{
	// good calls
	OP_SPHERES, OP_LEVEL, OP_FRAME, OP_CONFIG, OP_SUBMIT, OP_WAIT, OP_READY, OP_UPSCALE, OP_STATS,
	// refusals
	R_LEVEL_PORTALS, R_LEVEL_TEXT, R_LEVEL_PATH, R_SPH_MANY, R_SPH_BIG, R_UP_SCALE0, R_UP_PITCH, R_PROBE, R_PLANE, R_ORDER, R_OPT_UNKNOWN,
	R_HOSTREG, R_CONFIG, R_SUBMIT_SLOT, R_TRACE_CAM,
	R_SUBMIT_BUSY, R_WAIT_NEVER,                        // (with an argument: the slot)
	R_UP_NULL, R_OPT_BLUR2, R_TRACE_BUSY, R_NOTSUP,    // a group's own rules
	OP_COUNT
};
static const char *const OP_NAME[OP_COUNT] = { "upload_spheres", "level_load_mem", "trace_screen_centred", "frames_config", "submit_frame", "wait_frame", "frame_ready",
	"screen_upscale", "get_stats", "upload_level(bad portal map)", "level_load_mem(NULL)", "level_load(missing)", "upload_spheres(OBJ_MAX+1)", "upload_spheres(too big)",
	"screen_upscale(scale 0)", "screen_upscale(small pitch)", "probe(op 9999)", "read_plane(NULL)", "unit_order_probe(0 units)", "set_option(9999)", "host_register(NULL)",
	"frames_config(bad flags)", "submit_frame(bad slot)", "trace_screen_centred(NULL cam)", "submit_frame(busy slot)", "wait_frame(never submitted)",
	"screen_upscale(NULL) before a frame", "set_option(BLUR_PASSES, 2)", "trace_screen_centred with frames in flight", "pwn_tiled_* / strip forms" };
// what the header states for each refusal (the one-context handle must give it too, or the step tests nothing)
static int op_code(int op)
{
	if(op < R_LEVEL_PORTALS) return PWN_OK;
	return op == R_LEVEL_PATH ? PWN_EIO : op == R_SPH_BIG ? PWN_ETOOBIG : (op == R_SUBMIT_BUSY || op == R_TRACE_BUSY) ? PWN_EBUSY : op == R_NOTSUP ? PWN_ENOTSUP : PWN_EINVAL;
}
static bool own_rule(int op) { return op >= R_UP_NULL; }

struct step_t { int op, a; };
struct rec_t { int rc; unsigned long long hash; bool operator!=(const rec_t &o) const { return rc != o.rc || hash != o.hash; } };
static unsigned long long fnv(unsigned long long h, const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for(size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull; return h; }

static const char *LEVEL2 =
	"###########\r\n#;;;;;;;;;#\r\n#;;*;;$;;;#\r\n#;;;;;;;;;#\r\n#;a;;;;;b;#\r\n#;;;$;;;;;#\r\n###########\r\n";
static uint8_t g_cells[4096]; static pwn_portal g_pmap[26], g_bad_pmap[26];
static std::vector<pwn_sphere> g_too_big;

struct hnd_t
{
	pwn_ctx *ctx; int members, w, h;
	std::vector<uint32_t> sb, up; std::vector<float> zb;
};

static void info_of(pwn_ctx *ctx, pwn_group_info *gi) { if(pwn_group_info_get(ctx, gi) != PWN_OK) { fprintf(stderr, "pwn_group_info_get failed\n"); exit(1); } }
static bool info_same(const pwn_group_info &a, const pwn_group_info &b)
{
	return a.transport == b.transport && strcmp(a.note, b.note) == 0 && memcmp(a.cuts, b.cuts, sizeof(a.cuts)) == 0 && a.halo_rows == b.halo_rows && a.host_sink == b.host_sink && a.frames == b.frames;
}

static rec_t do_step(hnd_t &H, const step_t &s)
{
	pwn_ctx *ctx = H.ctx;
	const bool grp = H.members > 1;
	const size_t n = (size_t)H.w * H.h;
	rec_t r = { PWN_OK, 14695981039346656037ull };
	std::vector<pwn_sphere> sph;
	float cam[16];
	if(own_rule(s.op) && !grp) { r.rc = op_code(s.op); return r; }
	switch(s.op)
	{
		case OP_SPHERES: spheres_for(sph, s.a); r.rc = pwn_upload_spheres(ctx, sph.data(), (int)sph.size()); break;
		case OP_LEVEL: { const char *t = s.a ? LEVEL2 : LEVEL; r.rc = pwn_level_load_mem(ctx, t, (int)strlen(t)); break; }
		case OP_FRAME:
			cam_for(cam, s.a);
			r.rc = pwn_trace_screen_centred(ctx, cam, sec_for(s.a), H.sb.data(), H.zb.data());
			r.hash = fnv(fnv(r.hash, H.sb.data(), n * 4), H.zb.data(), n * 4);
			break;
		case OP_CONFIG: r.rc = s.a < 0 ? pwn_frames_config(ctx, 0, 0, 1, 0) : pwn_frames_config(ctx, 3, s.a, 1, 0); break;
		case OP_SUBMIT: case R_SUBMIT_BUSY: cam_for(cam, s.a >> 4); r.rc = pwn_submit_frame(ctx, cam, sec_for(s.a >> 4), s.a & 15); break;
		case OP_WAIT: case R_WAIT_NEVER:
		{
			pwn_frame fr;
			memset(&fr, 0x5a, sizeof(fr));
			const pwn_frame untouched = fr;
			r.rc = pwn_wait_frame(ctx, s.a, &fr);
			if(r.rc != PWN_OK) { r.hash = fnv(r.hash, "untouched", memcmp(&fr, &untouched, sizeof(fr)) == 0 ? 9 : 2); break; }
			// (every plane the frame's flags promise; a frame left on the device is read from there)
			r.hash = fnv(fnv(r.hash, &fr.seq, sizeof(fr.seq)), &fr.sec_current, sizeof(fr.sec_current));
			if(fr.sbuf != NULL) r.hash = fnv(r.hash, fr.sbuf, n * 4);
			if(fr.zbuf != NULL) r.hash = fnv(r.hash, fr.zbuf, n * 4);
			if(fr.sbuf == NULL)
			{
				std::vector<uint32_t> tmp(n, 0u);
				const int rc = fr.d_sbuf != NULL ? pwn_read_plane(ctx, fr.d_sbuf, tmp.data(), n * 4) : PWN_EINVAL;
				r.hash = fnv(fnv(r.hash, &rc, sizeof(rc)), tmp.data(), n * 4);
			}
			break;
		}
		case OP_READY: r.rc = pwn_frame_ready(ctx, s.a); break;
		case OP_UPSCALE: r.rc = pwn_screen_upscale(ctx, H.sb.data(), 2, H.w * 8, H.up.data()); break;
		case OP_STATS: { pwn_stats st; r.rc = pwn_get_stats(ctx, &st); break; }
		case R_LEVEL_PORTALS: r.rc = pwn_upload_level(ctx, g_cells, g_bad_pmap); break;
		case R_LEVEL_TEXT: r.rc = pwn_level_load_mem(ctx, NULL, 10); break;
		case R_LEVEL_PATH: r.rc = pwn_level_load(ctx, "/nonexistent/level.txt"); break;
		case R_SPH_MANY: sph.resize((size_t)PWN_OBJ_MAX + 1); r.rc = pwn_upload_spheres(ctx, sph.data(), PWN_OBJ_MAX + 1); break;
		case R_SPH_BIG: r.rc = pwn_upload_spheres(ctx, g_too_big.data(), (int)g_too_big.size()); break;
		case R_UP_SCALE0: r.rc = pwn_screen_upscale(ctx, H.sb.data(), 0, H.w * 8, H.up.data()); break;
		case R_UP_PITCH: r.rc = pwn_screen_upscale(ctx, H.sb.data(), 2, H.w * 8 - 4, H.up.data()); break;
		case R_UP_NULL: r.rc = pwn_screen_upscale(ctx, NULL, 2, H.w * 8, H.up.data()); break;
		case R_PROBE: { uint32_t in[4] = { 1, 2, 3, 4 }, out[4] = { 0, 0, 0, 0 }; r.rc = pwn_probe(ctx, 9999, in, out, 1); r.hash = fnv(r.hash, out, sizeof(out)); break; }
		case R_PLANE: r.rc = pwn_read_plane(ctx, NULL, H.up.data(), 64); break;
		case R_ORDER: { uint16_t cost[4] = { 1, 2, 3, 4 }; uint32_t perm[4] = { 0, 0, 0, 0 }; r.rc = pwn_unit_order_probe(ctx, cost, 0, perm); r.hash = fnv(r.hash, perm, sizeof(perm)); break; }
		case R_OPT_UNKNOWN: r.rc = pwn_set_option(ctx, 9999, 1); break;
		case R_OPT_BLUR2: r.rc = pwn_set_option(ctx, PWN_OPT_BLUR_PASSES, 2); break;
		case R_HOSTREG: r.rc = pwn_host_register(ctx, NULL, 4096); break;
		case R_CONFIG: r.rc = pwn_frames_config(ctx, 3, 64, 1, 0); break;
		case R_SUBMIT_SLOT: cam_for(cam, 0); r.rc = pwn_submit_frame(ctx, cam, 0.5f, PWN_MAX_SLOTS); break;
		case R_TRACE_CAM: r.rc = pwn_trace_screen_centred(ctx, NULL, 0.5f, H.sb.data(), H.zb.data()); r.hash = fnv(fnv(r.hash, H.sb.data(), n * 4), H.zb.data(), n * 4); break;
		case R_TRACE_BUSY: cam_for(cam, 0); r.rc = pwn_trace_screen_centred(ctx, cam, 0.5f, H.sb.data(), H.zb.data()); r.hash = fnv(fnv(r.hash, H.sb.data(), n * 4), H.zb.data(), n * 4); break;
		case R_NOTSUP:
		{
			pwn_tiled_frame tf;
			cam_for(cam, 0);
			const int rcs[4] = { pwn_tiled_submit(ctx, cam, 0.5f), pwn_tiled_wait(ctx, 0, &tf), pwn_trace_rows_device(ctx, cam, 0.5f, 0, 8, H.sb.data(), H.zb.data(), NULL),
				pwn_blur_rows_device(ctx, 0, 8, H.sb.data(), H.zb.data(), H.up.data(), NULL) };
			r.rc = PWN_ENOTSUP;
			for(int i = 0; i < 4; i++) if(rcs[i] != PWN_ENOTSUP) r.rc = rcs[i] == PWN_OK ? 1 : rcs[i];
			break;
		}
	}
	if(s.op == OP_UPSCALE || (s.op >= R_UP_SCALE0 && s.op <= R_PLANE) || s.op == R_UP_NULL) r.hash = fnv(r.hash, H.up.data(), H.up.size() * 4);
	// (the blocking call's own rule on a group, where one context goes on: taken for a refusal of the group's)
	if(own_rule(s.op) && r.rc == op_code(s.op)) r.hash = 14695981039346656037ull;
	return r;
}

// runs the script on a fresh handle of `members` members (1: pwn_init); over every refused step a group's info stays as it was
static int run_script(int members, bool distinct, const std::vector<step_t> &script, std::vector<rec_t> &out, char *why, size_t why_n)
{
	const int w = 64, h = 160;
	hnd_t H;
	H.ctx = NULL; H.members = members; H.w = w; H.h = h;
	H.sb.assign((size_t)w * h, 0x11111111u); H.zb.assign((size_t)w * h, -3.0f); H.up.assign((size_t)w * h * 4, 0x22222222u);
	pwn_ctx *ctx = NULL;
	int devs[8];
	for(int i = 0; i < members; i++) devs[i] = distinct ? i : 0;
	if(members == 1) CK(pwn_init(&ctx, 0, w, h)); else CK(pwn_init_multi(&ctx, devs, members, w, h));
	H.ctx = ctx;
	int bad = 0;
	out.clear();
	for(size_t k = 0; k < script.size() && !bad; k++)
	{
		const step_t &s = script[k];
		pwn_group_info before, after;
		const bool refusal = s.op >= R_LEVEL_PORTALS;
		if(members > 1) info_of(ctx, &before);
		const rec_t r = do_step(H, s);
		out.push_back(r);
		// (a good call that is refused for the state the handle is in -- a frame before a level -- is a refusal like the others)
		if(members > 1 && r.rc < 0 && !refusal)
		{
			info_of(ctx, &after);
			if(!info_same(before, after)) { snprintf(why, why_n, "step %zu, %s -> %d: the group's info changed", k, OP_NAME[s.op], r.rc); bad = 1; }
		}
		if(members > 1 && r.rc < 0 && strstr(pwn_last_error(ctx), "member ") != NULL) { snprintf(why, why_n, "step %zu, %s -> %d: reported as a member's failure (%s)", k, OP_NAME[s.op], r.rc, pwn_last_error(ctx)); bad = 1; }
		if(refusal && members == 1 && r.rc != op_code(s.op)) { snprintf(why, why_n, "step %zu, %s: one context answers %d, the header says %d", k, OP_NAME[s.op], r.rc, op_code(s.op)); bad = 1; }
		if(refusal && members > 1)
		{
			info_of(ctx, &after);
			if(!info_same(before, after)) { snprintf(why, why_n, "step %zu, %s: the group's info changed (transport %d/%d halo %d/%d sink %d/%d frames %llu/%llu)", k, OP_NAME[s.op], before.transport, after.transport, before.halo_rows, after.halo_rows, before.host_sink, after.host_sink, (unsigned long long)before.frames, (unsigned long long)after.frames); bad = 1; }
		}
	}
	pwn_destroy(ctx);
	return bad;
}

static int same_transcript(const std::vector<step_t> &script, const std::vector<rec_t> &one, const std::vector<rec_t> &grp, char *why, size_t why_n)
{
	for(size_t k = 0; k < script.size(); k++)
		if(k >= one.size() || k >= grp.size() || one[k] != grp[k])
		{
			if(k < one.size() && k < grp.size()) snprintf(why, why_n, "step %zu, %s(%d): one context %d / %016llx, the group %d / %016llx", k, OP_NAME[script[k].op], script[k].a, one[k].rc, one[k].hash, grp[k].rc, grp[k].hash);
			else snprintf(why, why_n, "step %zu: a transcript ends", k);
			return 1;
		}
	return 0;
}

// the states a refusal is tried in, and what follows it
enum { S_NO_LEVEL, S_LEVEL, S_BLOCKING, S_RESIDENT, S_FLIGHT1_SINK, S_FLIGHT2_SINK, S_FLIGHT3_SINK, S_FLIGHT1_RES, S_FLIGHT2_RES, S_FLIGHT3_RES, S_COUNT };
static const char *const S_NAME[S_COUNT] = { "no level", "level, no frame", "after a blocking frame", "after a resident frame", "1 in flight (sink)", "2 in flight (sink)",
	"3 in flight (sink)", "1 in flight (resident)", "2 in flight (resident)", "3 in flight (resident)" };

// appends: the state is set up, the refusal made, then every slot's wait and one blocking frame.  false, and nothing appended: the call is
// no refusal in this state (or cannot be made).  `fresh`: no blocking frame was delivered on the handle yet
static bool scripted(int state, int refusal, bool fresh, std::vector<step_t> &s)
{
	const int flight = state >= S_FLIGHT1_RES ? state - S_FLIGHT1_RES + 1 : state >= S_FLIGHT1_SINK ? state - S_FLIGHT1_SINK + 1 : 0;
	const bool slots = flight > 0 || state == S_RESIDENT;
	if(refusal == R_SUBMIT_BUSY && flight == 0) return false;
	if(refusal == R_TRACE_BUSY && flight == 0) return false;
	if(refusal == R_UP_NULL && (!fresh || state == S_BLOCKING)) return false;       // (a frame was delivered: no refusal)
	if(state != S_NO_LEVEL && s.empty()) { s.push_back({ OP_LEVEL, 0 }); s.push_back({ OP_SPHERES, 1 }); }
	if(state == S_NO_LEVEL && s.empty()) s.push_back({ OP_CONFIG, PWN_FRAME_SBUF | PWN_FRAME_ZBUF });
	if(state == S_BLOCKING && s.size() == 2) s.push_back({ OP_FRAME, 3 });            // (later: the frame that followed the refusal before)
	if(slots) s.push_back({ OP_CONFIG, (state == S_RESIDENT || state >= S_FLIGHT1_RES) ? 0 : (PWN_FRAME_SBUF | PWN_FRAME_ZBUF) });
	if(state == S_RESIDENT) { s.push_back({ OP_SUBMIT, (21 << 4) | 0 }); s.push_back({ OP_WAIT, 0 }); }
	// (slots that are made afresh: nothing counts as submitted to them, whatever was before)
	if(state == S_RESIDENT && refusal == R_WAIT_NEVER) s.push_back({ OP_CONFIG, 0 });
	for(int f = 0; f < flight; f++) { s.push_back({ OP_SPHERES, f }); s.push_back({ OP_SUBMIT, ((18 + f) << 4) | f }); }       // (frame 20: the deep band that leaves the halo)
	s.push_back({ refusal, refusal == R_SUBMIT_BUSY ? ((5 << 4) | (flight - 1)) : refusal == R_WAIT_NEVER ? (state == S_RESIDENT ? 0 : slots && flight < 3 ? 2 : slots ? 3 : 0) : 0 });
	// then, behind a refused level, the good one loads (the host's fallback, level.h:110-115); every slot's wait (a slot nothing was
	// submitted to: a refusal again), and one blocking frame
	if(refusal <= R_LEVEL_PATH && state != S_NO_LEVEL) s.push_back({ OP_LEVEL, 1 });
	// (no level: a submit is refused like the blocking call, and nothing counts as submitted)
	if(state == S_NO_LEVEL) { s.push_back({ OP_SUBMIT, (3 << 4) | 1 }); s.push_back({ R_WAIT_NEVER, 1 }); }
	for(int f = 0; f < 3 && flight > 0; f++) { if(f == 1 && flight >= 2) s.push_back({ OP_READY, 1 }); s.push_back({ f < flight ? OP_WAIT : R_WAIT_NEVER, f }); }
	s.push_back({ OP_FRAME, refusal % 4 == 0 ? 22 : 4 + refusal % 4 });
	return true;
}

// a sequence of 40 calls, good ones and refusals, as a small model of the handle allows them
static void seeded(unsigned seed, std::vector<step_t> &s)
{
	unsigned rs = seed * 2654435761u + 12345u;
	auto rnd = [&rs](unsigned n) { rs = rs * 1664525u + 1013904223u; return (rs >> 10) % n; };
	bool level = false, blocking = false; int nslots = 0, flags = 0, fifo[3], nfifo = 0, f = (int)rnd(8); bool submitted[3] = { false, false, false };
	s.clear();
	if(rnd(4) != 0) { s.push_back({ OP_LEVEL, 0 }); level = true; }
	while(s.size() < 40)
	{
		auto in_flight = [&](int slot) { for(int i = 0; i < nfifo; i++) if(fifo[i] == slot) return true; return false; };
		if(rnd(100) < 35)
		{
			const int r = R_LEVEL_PORTALS + (int)rnd(OP_COUNT - R_LEVEL_PORTALS);
			if(r == R_SPH_BIG && rnd(4) != 0) continue;             // (the one costly call)
			if(r == R_SUBMIT_BUSY) { if(nfifo == 0) continue; s.push_back({ r, ((f % 30) << 4) | fifo[rnd(nfifo)] }); continue; }
			if(r == R_WAIT_NEVER) { int slot = nslots; for(int i = 0; i < nslots; i++) if(!submitted[i]) slot = i; s.push_back({ r, slot }); continue; }
			if(r == R_TRACE_BUSY && nfifo == 0) continue;
			if(r == R_UP_NULL && blocking) continue;
			s.push_back({ r, 0 });
			continue;
		}
		switch(rnd(9))
		{
			case 0: s.push_back({ OP_SPHERES, (int)rnd(30) }); break;
			case 1: if(rnd(3) == 0) { s.push_back({ OP_LEVEL, (int)rnd(2) }); level = true; } break;
			case 2: if(nfifo == 0) { s.push_back({ OP_FRAME, f++ % 30 }); if(level) blocking = true; } break;
			case 3: if(nfifo == 0 && rnd(3) == 0) { flags = rnd(2) ? (PWN_FRAME_SBUF | PWN_FRAME_ZBUF) : 0; nslots = 3; s.push_back({ OP_CONFIG, flags }); submitted[0] = submitted[1] = submitted[2] = false; } break;
			case 4: case 5:
				for(int slot = 0; slot < nslots; slot++)
					if(!in_flight(slot)) { s.push_back({ OP_SUBMIT, ((f++ % 30) << 4) | slot }); if(level) { fifo[nfifo++] = slot; submitted[slot] = true; } break; }
				break;
			case 6:
				if(nfifo > 0)
				{
					// (frames left on the devices are looked at in the order they were submitted: a later frame's gather may reuse the plane)
					const int k = flags ? (int)rnd(nfifo) : 0;
					s.push_back({ OP_WAIT, fifo[k] });
					for(int i = k + 1; i < nfifo; i++) fifo[i - 1] = fifo[i];
					nfifo--;
				}
				break;
			case 7: if(nslots > 0) s.push_back({ OP_READY, (int)rnd(nslots) }); else if(blocking) s.push_back({ OP_UPSCALE, 0 }); break;
			case 8: s.push_back({ OP_STATS, 0 }); break;
		}
	}
	while(nfifo > 0) { s.push_back({ OP_WAIT, fifo[0] }); for(int i = 1; i < nfifo; i++) fifo[i - 1] = fifo[i]; nfifo--; }
	s.push_back({ OP_FRAME, f % 30 });
}

static const unsigned SEEDS[] = { 1, 2, 3, 5, 8, 13 };

static int refusals(const char *only_seed)
{
	pwn_ctx *ctx = NULL;
	// the good level's tables with one portal record overwritten (pwn_check_portals: a coordinate beyond 63), and spheres whose lists no form of the tables holds
	CK(pwn_init(&ctx, 0, 64, 160));
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_get_level(ctx, g_cells, g_pmap, NULL));
	pwn_destroy(ctx); ctx = NULL;
	memcpy(g_bad_pmap, g_pmap, sizeof(g_pmap));
	memset(&g_bad_pmap[7], 0x7f, sizeof(pwn_portal));
	g_too_big.clear();
	for(int i = 0; i <= PWN_LIST_MAX; i++) { pwn_sphere q = { 0.1f, 0.5f, 2.5f, 0.4f, 2.5f, 0.3f, 0.6f, 0.9f }; g_too_big.push_back(q); }      // (one cell's list beyond PWN_LIST_MAX)
	const struct { int members; bool distinct; } groups[] = { { 2, false }, { 3, false }, { 5, false }, { 3, true } };
	int bad = 0, scripts = 0, steps = 0;
	char why[400];
	std::vector<step_t> script;
	std::vector<rec_t> one, got;
	// "level, no frame": a fresh handle for every refusal; every other state is set up again on the same handle, refusal after refusal
	// (the group's own refusal of pwn_screen_upscale(NULL), which needs a handle without a delivered frame, first)
	for(int state = 0; state < S_COUNT && only_seed == NULL; state++)
		for(int r = R_LEVEL_PORTALS; r < OP_COUNT; r++)
		{
			if(state == S_LEVEL) { script.clear(); if(!scripted(state, r, true, script)) continue; }
			else
			{
				if(r != R_LEVEL_PORTALS) break;
				script.clear();
				bool fresh = true;
				for(int k = R_LEVEL_PORTALS - 1; k < OP_COUNT; k++)
				{
					const int q = k < R_LEVEL_PORTALS ? R_UP_NULL : k;
					if((q == R_UP_NULL && k >= R_LEVEL_PORTALS) || !scripted(state, q, fresh, script)) continue;
					fresh = state == S_NO_LEVEL;
				}
			}
			why[0] = 0;
			int b = run_script(1, false, script, one, why, sizeof(why));
			for(size_t gi = 0; gi < sizeof(groups) / sizeof(groups[0]) && !b; gi++)
			{
				b = run_script(groups[gi].members, groups[gi].distinct, script, got, why, sizeof(why)) || same_transcript(script, one, got, why, sizeof(why));
				if(b) fprintf(stderr, "refusals: state \"%s\", %d members%s: %s\n", S_NAME[state], groups[gi].members, groups[gi].distinct ? " on devices of their own" : "", why);
			}
			if(b && why[0] && one.size() < script.size()) fprintf(stderr, "refusals: state \"%s\", one context: %s\n", S_NAME[state], why);
			bad |= b; scripts++; steps += (int)script.size();
		}
	for(size_t k = 0; k < sizeof(SEEDS) / sizeof(SEEDS[0]); k++)
	{
		const unsigned seed = only_seed != NULL ? (unsigned)strtoul(only_seed, NULL, 10) : SEEDS[k];
		seeded(seed, script);
		why[0] = 0;
		int b = run_script(1, false, script, one, why, sizeof(why));
		if(b) fprintf(stderr, "refusals: seed %u, one context: %s\n", seed, why);
		for(size_t gi = 0; gi < sizeof(groups) / sizeof(groups[0]) && !b; gi++)
		{
			b = run_script(groups[gi].members, groups[gi].distinct, script, got, why, sizeof(why)) || same_transcript(script, one, got, why, sizeof(why));
			if(b) fprintf(stderr, "refusals: seed %u (replay: refusals %u), %d members%s: %s\n", seed, seed, groups[gi].members, groups[gi].distinct ? " on devices of their own" : "", why);
		}
		bad |= b; scripts++; steps += (int)script.size();
		if(only_seed != NULL) break;
	}
	printf("refusals: %d scripts, %d steps, each on one context and on groups of 2, 3, 5 on one device and of 3 on devices of their own: %s\n", scripts, steps, bad ? "FAILED" : "the same return codes and the same bits, a group's info unchanged over every refused call");
	return bad;
}

// ---- lost: a real failure with frames in flight is every lost slot's, once; then the handle renders one context's frames again ------
extern "C" long fakehip_alloc_fail_in;          // fake_hip.cpp: the k-th allocation from now fails (counted down atomically: the members allocate on their own threads)

// frames f0 .. f0+2 through three slots of a handle whose level and spheres are set: what a fresh one context delivers
static int three_frames(pwn_ctx *ctx, int w, int h, int f0, std::vector<std::vector<uint32_t>> &sb, std::vector<std::vector<float>> &zb)
{
	const size_t n = (size_t)w * h;
	float cam[16];
	sb.clear(); zb.clear();
	for(int f = 0; f < 3; f++) { cam_for(cam, f0 + f); CK(pwn_submit_frame(ctx, cam, sec_for(f0 + f), f)); }
	for(int f = 0; f < 3; f++)
	{
		pwn_frame fr;
		if(pwn_frame_ready(ctx, f) < 0) { fprintf(stderr, "lost: pwn_frame_ready(%d) of a fresh frame is negative (%s)\n", f, pwn_last_error(ctx)); return 1; }
		CK(pwn_wait_frame(ctx, f, &fr));
		if(fr.sbuf == NULL || fr.zbuf == NULL) { fprintf(stderr, "lost: PWN_OK with NULL planes\n"); return 1; }
		sb.push_back(std::vector<uint32_t>(fr.sbuf, fr.sbuf + n)); zb.push_back(std::vector<float>(fr.zbuf, fr.zbuf + n));
	}
	return 0;
}

static bool same_planes(const std::vector<std::vector<uint32_t>> &a, const std::vector<std::vector<float>> &az, const std::vector<std::vector<uint32_t>> &b, const std::vector<std::vector<float>> &bz)
{
	if(a.size() != b.size() || az.size() != bz.size()) return false;
	for(size_t f = 0; f < a.size(); f++) if(a[f] != b[f] || memcmp(az[f].data(), bz[f].data(), az[f].size() * 4) != 0) return false;
	return true;
}

// member 1 is 0.9 s late to the second submit of three, wait deadline 0.2 s (the `late` mode's numbers)
static int lost_late(void)
{
	const int w = 64, h = 96, flags = PWN_FRAME_SBUF | PWN_FRAME_ZBUF;
	pwn_ctx *ctx = NULL;
	std::vector<pwn_sphere> sph;
	spheres_for(sph, 1);
	// one context, fresh: the three frames a host submits once the failure is dealt with (a tiling that was taken down comes up with
	// its depth planes at zero, like slots after pwn_frames_config)
	std::vector<std::vector<uint32_t>> ref, got; std::vector<std::vector<float>> zref, zgot;
	CK(pwn_init(&ctx, 0, w, h));
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_upload_spheres(ctx, sph.data(), (int)sph.size()));
	CK(pwn_frames_config(ctx, 3, flags, 1, 0));
	if(three_frames(ctx, w, h, 4, ref, zref)) return 1;
	pwn_destroy(ctx); ctx = NULL;

	int devs[3] = { 0, 0, 0 };
	setenv("PWN_DBG_GROUP_STALL", "1:2:900:submit", 1);
	CK(pwn_init_multi(&ctx, devs, 3, w, h));
	unsetenv("PWN_DBG_GROUP_STALL");
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_upload_spheres(ctx, sph.data(), (int)sph.size()));
	CK(pwn_tiled_set_timeouts(ctx, 5000, 200));
	CK(pwn_frames_config(ctx, 3, flags, 1, 0));
	float cam[16];
	for(int f = 0; f < 3; f++) { cam_for(cam, f); CK(pwn_submit_frame(ctx, cam, sec_for(f), f)); }
	int bad = 0, lost = 0;
	for(int f = 0; f < 3; f++)
	{
		pwn_frame fr;
		memset(&fr, 0x5a, sizeof(fr));
		const pwn_frame untouched = fr;
		const int rc = pwn_wait_frame(ctx, f, &fr);
		if(rc == PWN_OK) { if(fr.sbuf == NULL || fr.zbuf == NULL) { fprintf(stderr, "lost: slot %d: PWN_OK with NULL planes (seq %llu)\n", f, (unsigned long long)fr.seq); bad = 1; } continue; }
		lost++;
		printf("lost: wait of slot %d -> %d (%s)\n", f, rc, pwn_last_error(ctx));
		if(strstr(pwn_last_error(ctx), "member") == NULL) { fprintf(stderr, "lost: slot %d: the error names no member\n", f); bad = 1; }
		if(memcmp(&fr, &untouched, sizeof(fr)) != 0) { fprintf(stderr, "lost: slot %d: *out was written\n", f); bad = 1; }
		// the slots behind it: lost too, and pwn_frame_ready says so
		for(int k = f + 1; k < 3; k++) { const int q = pwn_frame_ready(ctx, k); if(q >= 0) { fprintf(stderr, "lost: pwn_frame_ready(%d) -> %d behind a lost frame\n", k, q); bad = 1; } }
		// once: the slot is free, as if never submitted
		const int again = pwn_wait_frame(ctx, f, &fr);
		if(again != PWN_EINVAL) { fprintf(stderr, "lost: slot %d: a second wait -> %d, not PWN_EINVAL\n", f, again); bad = 1; }
		const int free_now = pwn_frame_ready(ctx, f);
		if(free_now != 1) { fprintf(stderr, "lost: slot %d: pwn_frame_ready -> %d once the loss was reported, not 1 (nothing in flight)\n", f, free_now); bad = 1; }
	}
	if(lost != 3) { fprintf(stderr, "lost: %d slots reported lost, expected all three (the late member holds the second submit back, the first frame's wait is behind it)\n", lost); bad = 1; }
	if(!bad && three_frames(ctx, w, h, 4, got, zgot)) bad = 1;
	if(!bad && !same_planes(ref, zref, got, zgot)) { fprintf(stderr, "lost: the three frames after the failure differ from one context's\n"); bad = 1; }
	pwn_destroy(ctx);
	printf("lost: late member: %s\n", bad ? "FAILED" : "every lost slot's wait failed once, naming a member; three fresh frames equal one context's");
	return bad;
}

// one member cannot allocate for a posted sphere upload (PWN_ENOMEM): the next call that waits says so, a repeated upload mends it
static int lost_upload(bool in_flight, bool first_frame)
{
	const int w = 64, h = 96, flags = PWN_FRAME_SBUF | PWN_FRAME_ZBUF;
	const size_t n = (size_t)w * h;
	pwn_ctx *one = NULL, *ctx = NULL;
	std::vector<pwn_sphere> small, big;
	spheres_for(small, 1);
	// (so many small spheres that their lists go to device memory: the upload allocates)
	unsigned rs = 777;
	auto rnd = [&rs]() { rs = rs * 1664525u + 1013904223u; return (float)(rs >> 8) / 16777216.0f; };
	for(int i = 0; i < 2100; i++) { pwn_sphere q = { 0.02f + 0.06f * rnd(), rnd(), 1.0f + 12.0f * rnd(), rnd(), 1.0f + 12.0f * rnd(), rnd(), rnd(), rnd() }; big.push_back(q); }
	float cam[16];
	std::vector<uint32_t> sb(n), rb(n); std::vector<float> zb(n), rz(n);
	int devs[3] = { 0, 0, 0 }, bad = 0;
	{ pwn_ctx *&ctx = one; CK(pwn_init(&ctx, 0, w, h)); CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL))); CK(pwn_upload_spheres(ctx, small.data(), (int)small.size())); }
	CK(pwn_init_multi(&ctx, devs, 3, w, h));
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_upload_spheres(ctx, small.data(), (int)small.size()));
	// a frame with the small tables, on both (or none: the upload then fails with the tiling still down)
	cam_for(cam, 0);
	if(first_frame)
	{
		CK(pwn_trace_screen_centred(ctx, cam, sec_for(0), sb.data(), zb.data()));
		{ pwn_ctx *&ctx = one; CK(pwn_trace_screen_centred(ctx, cam, sec_for(0), rb.data(), rz.data())); }
		if(sb != rb) { fprintf(stderr, "lost: upload: the first frame differs\n"); bad = 1; }
	}
	// one context with the tables last uploaded successfully: the only frames a wait may deliver with PWN_OK (made before the allocation
	// that fails is armed: the members allocate on their own threads, behind the call)
	std::vector<std::vector<uint32_t>> okf;
	if(in_flight) { pwn_ctx *&ctx = one; CK(pwn_frames_config(ctx, 3, flags, 1, 0)); for(int f = 0; f < 2; f++) { pwn_frame fr; cam_for(cam, 1 + f); CK(pwn_submit_frame(ctx, cam, sec_for(1 + f), f)); CK(pwn_wait_frame(ctx, f, &fr)); okf.push_back(std::vector<uint32_t>(fr.sbuf, fr.sbuf + n)); } }
	if(in_flight) { CK(pwn_frames_config(ctx, 3, flags, 1, 0)); cam_for(cam, 1); CK(pwn_submit_frame(ctx, cam, sec_for(1), 0)); }
	// the upload that one member cannot make: the call itself has nothing to report yet
	__atomic_store_n(&fakehip_alloc_fail_in, 1L, __ATOMIC_RELEASE);
	CK(pwn_upload_spheres(ctx, big.data(), (int)big.size()));
	int reported = 0;
	if(in_flight)
	{
		cam_for(cam, 2); CK(pwn_submit_frame(ctx, cam, sec_for(2), 1));
		for(int f = 0; f < 2; f++)
		{
			pwn_frame fr;
			const int rc = pwn_wait_frame(ctx, f, &fr);
			if(rc == PWN_OK) { if(fr.sbuf == NULL || std::vector<uint32_t>(fr.sbuf, fr.sbuf + n) != okf[(size_t)f]) { fprintf(stderr, "lost: upload: slot %d delivered with PWN_OK a frame that is not one context's for the tables last uploaded\n", f); bad = 1; } continue; }
			if(!reported) printf("lost: upload: wait of slot %d -> %d (%s)\n", f, rc, pwn_last_error(ctx));
			reported++;
			if(strstr(pwn_last_error(ctx), "member") == NULL) { fprintf(stderr, "lost: upload: the error names no member\n"); bad = 1; }
		}
	}
	else
	{
		cam_for(cam, 1);
		const int rc = pwn_trace_screen_centred(ctx, cam, sec_for(1), sb.data(), zb.data());
		printf("lost: upload: the next blocking call -> %d (%s)\n", rc, pwn_last_error(ctx));
		if(rc == PWN_OK) { fprintf(stderr, "lost: upload: the call after the failed upload returned PWN_OK\n"); bad = 1; }
		else { reported++; if(rc != PWN_ENOMEM || strstr(pwn_last_error(ctx), "member") == NULL) { fprintf(stderr, "lost: upload: expected PWN_ENOMEM naming a member\n"); bad = 1; } }
	}
	if(!reported) { fprintf(stderr, "lost: upload: no call reported the failed upload\n"); bad = 1; }
	__atomic_store_n(&fakehip_alloc_fail_in, 0L, __ATOMIC_RELEASE);
	pwn_destroy(one); one = NULL;
	// the host uploads again: from then on one context's frames (a fresh one: the tiling came up anew, depth planes at zero)
	{ pwn_ctx *&ctx = one; CK(pwn_init(&ctx, 0, w, h)); CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL))); CK(pwn_upload_spheres(ctx, big.data(), (int)big.size())); }
	CK(pwn_upload_spheres(ctx, big.data(), (int)big.size()));
	if(in_flight)
	{
		std::vector<std::vector<uint32_t>> ref, got; std::vector<std::vector<float>> zref, zgot;
		{ pwn_ctx *&ctx = one; CK(pwn_frames_config(ctx, 3, flags, 1, 0)); }
		if(three_frames(one, w, h, 5, ref, zref) || three_frames(ctx, w, h, 5, got, zgot)) bad = 1;
		else if(!same_planes(ref, zref, got, zgot)) { fprintf(stderr, "lost: upload: frames in flight after the repeated upload differ from one context's\n"); bad = 1; }
	}
	else for(int f = 3; f < 6 && !bad; f++)
	{
		cam_for(cam, f);
		CK(pwn_trace_screen_centred(ctx, cam, sec_for(f), sb.data(), zb.data()));
		{ pwn_ctx *&ctx = one; CK(pwn_trace_screen_centred(ctx, cam, sec_for(f), rb.data(), rz.data())); }
		if(sb != rb || memcmp(zb.data(), rz.data(), n * 4) != 0) { fprintf(stderr, "lost: upload: frame %d after the repeated upload differs from one context's\n", f); bad = 1; }
	}
	pwn_destroy(one);
	pwn_destroy(ctx);
	printf("lost: upload (%s): %s\n", in_flight ? "frames in flight" : first_frame ? "blocking calls" : "before the first frame", bad ? "FAILED" : "reported once, naming the member; after the repeated upload every frame equals one context's");
	return bad;
}

// members that disagree: member 1 alone refuses a call (it has a frame of its own in flight, made behind the group's back through
// pwn_internal.h's pwn_group_member, so PWN_OPT_FRAME_OVERLAP is PWN_EBUSY there and accepted by the others) -- the members are in
// different states, which is a failure: reported naming member 1, mended, and the next frame is the frame
static int lost_disagree(void)
{
	const int w = 64, h = 96;
	const size_t n = (size_t)w * h;
	pwn_ctx *ctx = NULL;
	int devs[3] = { 0, 0, 0 }, bad = 0;
	std::vector<pwn_sphere> sph;
	spheres_for(sph, 1);
	std::vector<uint32_t> sb(n), first(n); std::vector<float> zb(n);
	float cam[16];
	cam_for(cam, 0);
	CK(pwn_init_multi(&ctx, devs, 3, w, h));
	CK(pwn_level_load_mem(ctx, LEVEL, (int)strlen(LEVEL)));
	CK(pwn_upload_spheres(ctx, sph.data(), (int)sph.size()));
	CK(pwn_trace_screen_centred(ctx, cam, 0.5f, first.data(), zb.data()));
	pwn_ctx *m1 = pwn_group_member(ctx, 1);
	{ pwn_ctx *&ctx = m1; CK(pwn_frames_config(ctx, 1, 0, 1, 0)); CK(pwn_submit_frame(ctx, cam, 0.5f, 0)); }
	const int rc = pwn_set_option(ctx, PWN_OPT_FRAME_OVERLAP, 0);
	printf("lost: disagree: pwn_set_option -> %d (%s)\n", rc, pwn_last_error(ctx));
	if(rc != PWN_EBUSY || strstr(pwn_last_error(ctx), "member 1") == NULL) { fprintf(stderr, "lost: disagree: expected member 1's PWN_EBUSY as a failure of the group\n"); bad = 1; }
	{ pwn_ctx *&ctx = m1; pwn_frame fr; CK(pwn_wait_frame(ctx, 0, &fr)); CK(pwn_frames_config(ctx, 0, 0, 1, 0)); }
	CK(pwn_set_option(ctx, PWN_OPT_FRAME_OVERLAP, 0));
	CK(pwn_trace_screen_centred(ctx, cam, 0.5f, sb.data(), zb.data()));
	if(sb != first) { fprintf(stderr, "lost: disagree: the frame after the failure differs\n"); bad = 1; }
	pwn_destroy(ctx);
	printf("lost: disagree: %s\n", bad ? "FAILED" : "a call refused by one member only is a failure naming it; mended");
	return bad;
}

static int lost_frames(void) { int bad = lost_late(); bad |= lost_upload(false, true); bad |= lost_upload(false, false); bad |= lost_upload(true, true); bad |= lost_disagree(); return bad; }

int main(int argc, char **argv)
{
	setenv("PWN_GROUP_TRANSPORT", "local", 1);
	int bad = 0;
	const char *what = argc > 1 ? argv[1] : "all";
	if(!strcmp(what, "all") || !strcmp(what, "refusals")) bad |= refusals(argc > 2 ? argv[2] : NULL);
	if(!strcmp(what, "all") || !strcmp(what, "lost")) bad |= lost_frames();
	if(!strcmp(what, "all") || !strcmp(what, "group")) { bad |= group_runs(64, 160); bad |= group_runs(128, 96); }
	if(!strcmp(what, "all") || !strcmp(what, "late")) bad |= late_member();
	if(!strcmp(what, "all") || !strcmp(what, "shm")) { bad |= shm_ranks(2); bad |= shm_ranks(3); }
	printf(bad ? "FAILED\n" : "ok\n");
	return bad;
}

/* sphere_box_driver.c -- sphere_box.h (what the device's table builder computes a sphere's cells and r*r with) held to
   level_host.c's pwn_bin_spheres on the CPU (tests/test_sphere_box.py compiles both with gcc).
       sphere_box_driver SPHERES.bin      n records of pwn_sphere
   Per sphere: the cells of its box word are exactly the cells pwn_bin_spheres bins that sphere to, and r*r is the product the
   host packs (pwn_tables.cpp), flushed below FLT_MIN.  Over all spheres: the per-cell counts, and in every cell the order.
   Prints "pairs cells longest" of the box words, then "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pwnhip.h"
#include "level_host.h"
#include "sphere_box.h"

#define REQ(x, i) do { if(!(x)) { fprintf(stderr, "%s:%d: %s (sphere %d)\n", __FILE__, __LINE__, #x, (int)(i)); return 1; } } while(0)

int main(int argc, char **argv)
{
	if(argc != 2) return 2;
	FILE *fp = fopen(argv[1], "rb");
	if(fp == NULL) return 2;
	fseek(fp, 0, SEEK_END);
	const long bytes = ftell(fp);
	fseek(fp, 0, SEEK_SET);
	const int n = (int)(bytes / (long)sizeof(pwn_sphere));
	pwn_sphere *s = malloc(bytes > 0 ? (size_t)bytes : 1);
	if(fread(s, sizeof(pwn_sphere), (size_t)n, fp) != (size_t)n) return 2;
	fclose(fp);

	static int32_t off[4097], one[4097], cnt[4096];
	uint32_t *box = malloc(sizeof(uint32_t) * (size_t)(n > 0 ? n : 1));
	for(int i = 0; i < n; i++)
	{
		box[i] = pwn_box_pack(s[i].x, s[i].z, s[i].r);
		/* every field 0 .. 63 */
		REQ((box[i] & 0xc0c0c0c0u) == 0u, i);
		/* this sphere alone, binned by the host */
		int32_t idx[4096];
		const int m = pwn_bin_spheres(&s[i], 1, one, idx, 4096);
		REQ(m >= 0 && (uint32_t)m == pwn_box_cells(box[i]), i);
		for(int c = 0; c < 4096; c++)
			REQ((one[c + 1] - one[c] == 1) == (pwn_box_covers(box[i], (uint32_t)c & 63u, (uint32_t)c >> 6) != 0), i);
		/* r*r as pwn_i_pack_blob stores it */
		float r2 = s[i].r * s[i].r;
		if(r2 < 1.17549435e-38f) r2 = 0.0f;
		const float b2 = pwn_box_r2(s[i].r);
		REQ(memcmp(&r2, &b2, 4) == 0 || (r2 != r2 && b2 != b2), i);
		uint32_t u; memcpy(&u, &b2, 4);
		REQ((u & 0x7f800000u) != 0u || (u & 0x007fffffu) == 0u, i);          /* never a denormal */
	}
	/* all of them: the counts, and the order inside every cell */
	const int nb = pwn_bin_spheres(s, n, off, NULL, 0);
	REQ(nb >= 0, -1);
	int32_t *idx = malloc(sizeof(int32_t) * (size_t)(nb > 0 ? nb : 1));
	REQ(pwn_bin_spheres(s, n, off, idx, nb) == nb, -1);
	unsigned long long pairs = 0, cells = 0, longest = 0;
	for(int c = 0; c < 4096; c++)
	{
		int k = off[c];
		cnt[c] = 0;
		for(int i = 0; i < n; i++)
			if(pwn_box_covers(box[i], (uint32_t)c & 63u, (uint32_t)c >> 6)) { REQ(k < off[c + 1] && idx[k] == i, i); k++; cnt[c]++; }
		REQ(k == off[c + 1], c);
		pairs += (unsigned long long)cnt[c]; cells += cnt[c] != 0;
		if((unsigned long long)cnt[c] > longest) longest = (unsigned long long)cnt[c];
	}
	printf("%llu %llu %llu\nok\n", pairs, cells, longest);
	return 0;
}

/* level_bake_driver.c -- level_bake.h (the rules the device's level builder derives, checks and bakes a level with) held to
   level_host.c on the CPU (tests/test_level_bake.py compiles both with gcc, once plainly and once under AddressSanitizer + UBSan).
       level_bake_driver CASES.bin
   CASES.bin: int32 n, then n cases of int32 mode, 4096 cell bytes, 26 x 7 int32.  mode 1: the table is given; mode 0: it is derived
   from the cells and held to pwn_parse_level of those 4096 bytes; mode 2: derived, held to nothing but the bake (grids whose bytes
   mean something else to the parser).
   The algorithm is level_bake.hip's, one cell after the other: derive, verdict, and -- on verdict 0 ONLY -- the bake.  Per case one
   line: verdict letter host_check nrec host_nrec words_equal recs_equal table_equal, then the 182 words of the table used. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pwnhip.h"
#include "level_host.h"
#include "level_bake.h"

int main(int argc, char **argv)
{
	if(argc != 2) return 2;
	FILE *fp = fopen(argv[1], "rb");
	if(fp == NULL) return 2;
	int32_t n = 0;
	if(fread(&n, 4, 1, fp) != 1 || n < 0) return 2;
	for(int k = 0; k < n; k++)
	{
		int32_t mode;
		/* (the case's arrays to the byte, on the heap: a read or write beside them is a report) */
		uint8_t *cells = malloc(4096);
		int32_t *pmap = malloc(26 * PWN_LB_PM_WORDS * sizeof(int32_t));
		uint16_t *bits = malloc(65 * 65 * sizeof(uint16_t)), *hbits = malloc(65 * 65 * sizeof(uint16_t));
		uint32_t *recs = malloc(PWN_EP_MAX * sizeof(uint32_t)), *hrecs = malloc(PWN_EP_MAX * sizeof(uint32_t));
		if(fread(&mode, 4, 1, fp) != 1 || fread(cells, 1, 4096, fp) != 4096 || fread(pmap, 4, 26 * PWN_LB_PM_WORDS, fp) != 26 * PWN_LB_PM_WORDS) return 2;
		int table_equal = -1;
		if(mode != 1)
		{
			uint32_t first[26], second[26];
			for(int i = 0; i < 26; i++) first[i] = second[i] = 0xffffffffu;
			for(uint32_t cell = 0; cell < 4096u; cell++)
			{
				const int c = cells[cell];
				if(c < 'A' || c > 'Z') continue;
				if(first[c - 'A'] == 0xffffffffu) first[c - 'A'] = cell;
				else if(second[c - 'A'] == 0xffffffffu) second[c - 'A'] = cell;
			}
			for(int i = 0; i < 26; i++) pwn_lb_derive_letter(cells, first[i], second[i], pmap + PWN_LB_PM_WORDS * i);
			if(mode == 0)
			{
				uint8_t pcells[4096];
				pwn_portal ppm[26];
				int32_t spawn[2];
				if(pwn_parse_level((const char *)cells, 4096, pcells, ppm, spawn) != 0) return 3;
				table_equal = memcmp(ppm, pmap, sizeof(ppm)) == 0 && memcmp(pcells, cells, 4096) == 0;
			}
		}
		uint32_t bad1 = 26u, bad2 = 26u;
		for(int i = 25; i >= 0; i--) if(pwn_lb_coords_bad(pmap + PWN_LB_PM_WORDS * i)) bad1 = (uint32_t)i;
		for(int t = 0; t < 130; t++) { const int l = pwn_lb_outside_letter_nth(cells, pmap, t); if(l >= 0 && (uint32_t)l < bad2) bad2 = (uint32_t)l; }
		const int verdict = bad1 < 26u ? PWN_LB_BAD_COORD : (bad2 < 26u ? PWN_LB_BAD_OUTSIDE : PWN_LB_TAKEN);
		const uint32_t letter = verdict == PWN_LB_BAD_COORD ? bad1 : (verdict == PWN_LB_BAD_OUTSIDE ? bad2 : 26u);
		/* (the ruler reads a table's coordinates only behind its own range check) */
		const int host_check = pwn_check_portals(cells, (const pwn_portal *)pmap);
		int nrec = 0, hnrec = 0, words_equal = -1, recs_equal = -1;
		if(verdict == PWN_LB_TAKEN)
		{
			memset(bits, 0, 65 * 65 * sizeof(uint16_t));
			memset(recs, 0, PWN_EP_MAX * sizeof(uint32_t));
			for(int z = 0; z < 64; z++) for(int x = 0; x < 64; x++)
			{
				uint32_t inside, outside, rec = 0;
				const int c = cells[z * 64 + x];
				const int has = pwn_lb_cell_bits(c, x, z, pmap, (uint32_t)nrec, &inside, &outside, &rec);
				if(has != pwn_lb_is_endpoint(c, x, z, pmap)) return 4;
				if(has && nrec < (int)PWN_EP_MAX) recs[nrec++] = rec;
				bits[z * 65 + x] = (uint16_t)inside;
				if(x == 0) bits[z * 65 + 64] = (uint16_t)outside;
				if(z == 0) bits[64 * 65 + x] = (uint16_t)outside;
				if(x == 0 && z == 0) bits[64 * 65 + 64] = (uint16_t)outside;
				if((inside | outside) > 0xffffu) return 4;
			}
			if(host_check)
			{
				hnrec = pwn_bake_cells(cells, (const pwn_portal *)pmap, hbits, hrecs);
				words_equal = memcmp(bits, hbits, 65 * 65 * sizeof(uint16_t)) == 0;
				recs_equal = memcmp(recs, hrecs, PWN_EP_MAX * sizeof(uint32_t)) == 0;
			}
		}
		printf("%d %u %d %d %d %d %d %d", verdict, letter, host_check, nrec, hnrec, words_equal, recs_equal, table_equal);
		for(int i = 0; i < 26 * PWN_LB_PM_WORDS; i++) printf(" %d", pmap[i]);
		printf("\n");
		free(cells); free(pmap); free(bits); free(hbits); free(recs); free(hrecs);
	}
	fclose(fp);
	printf("ok\n");
	return 0;
}

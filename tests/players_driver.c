/* players_driver.c -- host/player.c's pwn_player_step over a batch, for tests/players_model.py: n players x ticks, the key byte of
   pwn_players_step (bit i = field i of pwn_keys) unpacked, the arrays in the layout of the C ABI.  Built with host/Makefile's flags. */
#include <string.h>
#include "player.h"

void players_model_step(int n, int ticks, const uint8_t *keys, float tdiff, const uint8_t *cells, const int32_t *pmap,
	float *cams, float *gravity, int32_t *traversals)
{
	pwn_portal pm[26];
	memcpy(pm, pmap, sizeof(pm));
	for(int i = 0; i < n; i++)
	{
		pwn_player p;
		const int b = keys[i];
		const pwn_keys k = { b & 1, (b >> 1) & 1, (b >> 2) & 1, (b >> 3) & 1, (b >> 4) & 1, (b >> 5) & 1, (b >> 6) & 1, (b >> 7) & 1 };
		memcpy(p.cam, cams + 16 * (size_t)i, sizeof(p.cam));
		memcpy(p.gravity, gravity + 4 * (size_t)i, sizeof(p.gravity));
		p.traversals = traversals != NULL ? traversals[i] : 0;
		for(int t = 0; t < ticks; t++) pwn_player_step(&p, &k, tdiff, cells, pm);
		memcpy(cams + 16 * (size_t)i, p.cam, sizeof(p.cam));
		memcpy(gravity + 4 * (size_t)i, p.gravity, sizeof(p.gravity));
		if(traversals != NULL) traversals[i] = p.traversals;
	}
}

// One sphere against the ray at `pos` (trace.h:256-294); textually included by trace_walk.inc inside each list form's loop.
// In scope: s0 = the record (x, y, z, r*r); PWN_ST_RAD2 = r*r as a float; PWN_ST_WHICH = what aux_idx remembers of the sphere;
// PWN_ST_OBJECT = the sphere's index in the live table (pwn_hit.object), evaluated only where WALK_HIDDEN asks for it (trace_walk.inc).
// A file of its own (not a macro) so that every instruction keeps a source line: tools/issue_model.py's regions (//@R).
//@R w_sphtest
{
	if(COUNT) cnt.tests++;
	V rel;
	rel.x = s0.x - pos.x; rel.y = s0.y - pos.y; rel.z = s0.z - pos.z;
	if constexpr(HAS_W) rel.w = 1.0f - pos.w; else rel.w = 0.0f;
	const float rad2 = PWN_ST_RAD2;
	float d2 = dot3<HAS_W>(rel, rel);
	float dt = dot3<HAS_W>(rel, ray);
	if(dt > 0.0f)
	{
		float calc = d2 - dt * dt;
		if(calc < rad2)
		{
			//@R w_sphhit
			WAVE_PATH(7);
			float sd2 = 1.0f - calc / rad2;
			float sdist = sqrtf(d2) - sqrtf(sd2);
			// (the hidden sphere of this view or ray, pwn_trace_*_hide_device: a candidate that would win and is that sphere changes no
			// state -- aux_dist, aux_pos, aux_diff and aux_idx stay, as if the table did not hold it.  Asked last, on the rare path:
			// which sphere a record is of is a table look-up in two of the three list forms.  Without HIDE the test is `false`.)
			if(sdist + cdist < aux_dist && !WALK_HIDDEN(PWN_ST_OBJECT))
			{
				//@R w_sphupd
				RG(RG_SPHUPD);
				aux_dist = sdist + cdist;
				if(aux_dist == -1.0f) aux_dist = __builtin_inff();
				aux_pos = vadd<HAS_W>(pos, vscale<HAS_W>(sdist, ray));
				V d;
				d.x = aux_pos.x - s0.x; d.y = aux_pos.y - s0.y; d.z = aux_pos.z - s0.z;
				if constexpr(HAS_W) d.w = aux_pos.w - 1.0f; else d.w = 0.0f;
				const V nrm = vnormalise<HAS_W>(L.rsq, d);
				float diff = -dot3<HAS_W>(ray, nrm);
				if(diff < 0.0f) diff = 0.0f;
				const float amb = 0.2f;
				aux_diff = amb + (1.0f - amb) * diff;
				aux_idx = PWN_ST_WHICH;
			}
			//@R w_sphhit
		}
		//@R w_sphtest
	}
}
